"""Chunked streaming inference with carried routing state.

``StreamingRouter(model, n_streams)`` feeds ``n_streams`` utterances to an evaluation-mode
``SequenceRouter`` chunk by chunk, in lock step, and emits every output frame as soon as
the input it depends on has arrived.  After ``finish()`` the concatenated logits are
those of ``model(all pushed feats, input_lengths=lens, training=False)``.

What an output frame needs of the future:

* CNN front end: output frame o reads input frames 4o .. 4o + 6 (two stride-2 3x3
  convolutions, TF "same" padding at a length that is a multiple of 4);
* primary capsules: frame o reads CNN-FE frames o - 1 .. o + 1 (the encaps 3x3);
* routing layer l: frame t reads its input frames t - lpad .. t + rpad (the window), and
  with sequential dynamic routing (SDR) its own output frame t - 1.

So after P pushed input frames P/4 - 1 CNN-FE frames are final, P/4 - 2 primary-capsule
frames and P/4 - 2 - l * rpad frames of routing layer l (``frames_final``): the model's
lookahead is 2 + L * rpad output frames.

State: the last 4 input frames; the CNN-FE frames the primary capsules still need; and per
routing layer a sliding buffer of its input frames (SDR: also of its output frames, for
the carry).  The routing buffers share one timeline -- local frame = global frame - base
-- so a layer's LayerNorm writes straight into the next layer's buffer, and one launch
(srf_stream_advance_n) slides them all.  Everything runs on the current stream under
``torch.no_grad()``: no side streams, no graph capture.

With a front end (``frontend=``, srf_amd/fbank.py) ``push_audio`` takes samples instead of
features.  The audio side adds its own lookahead: a feature frame
is final once the 4 frames after it are complete, 40 ms plus the frame's own 25 ms after
its first sample, and up to 3 final frames wait for their group of 4.
"""
import torch

from . import _lib, ctc, ops

_NO_END = 1 << 30   # length of a stream whose end is not known yet (device side)


def frames_final(pushed, n_layers, rpad, finished=False):
    """Output frames that are final per stage after ``pushed`` input frames (a multiple
    of 4): [CNN-FE, primary capsules, routing layer 1, ..., routing layer n_layers].  The
    last entry is what has been emitted.  ``finished``: the utterance ends at ``pushed``,
    every stage is complete."""
    if pushed % 4 or pushed < 0:
        raise ValueError(f'pushed frames must be a non-negative multiple of 4, got {pushed}')
    if finished:
        return [pushed // 4] * (n_layers + 2)
    out = [max(0, pushed // 4 - 1)]
    out.append(max(0, out[0] - 1))
    for _ in range(n_layers):
        out.append(max(0, out[-1] - rpad))
    return out


def stream_schedule(pushes, n_layers, rpad):
    """``frames_final`` after each push of ``pushes`` (input frames per chunk), then after
    ``finish()``: len(pushes) + 1 rows."""
    rows, total = [], 0
    for n in pushes:
        total += n
        rows.append(frames_final(total, n_layers, rpad))
    rows.append(frames_final(total, n_layers, rpad, finished=True))
    return rows


def check_ended(lengths, ended, pushed, n, unit='frames'):
    """Validate one push's ``ended`` against the streams' declared lengths (None: not
    declared) and return the new list.  ``pushed`` frames came before this chunk of
    ``n``; a declared length must lie in [pushed, pushed + n] and is declared once.
    ``unit`` names what is counted in the messages (the audio path counts samples)."""
    if ended is None:
        return list(lengths)
    vals = [int(e) for e in (ended.tolist() if hasattr(ended, 'tolist') else ended)]
    if len(vals) != len(lengths):
        raise ValueError(f'ended has {len(vals)} entries for {len(lengths)} streams')
    new = list(lengths)
    for b, e in enumerate(vals):
        if e == -1:
            continue
        if e < -1:
            raise ValueError(f'stream {b}: ended must be a length or -1, got {e}')
        if lengths[b] is not None:
            raise ValueError(f'stream {b}: its length was already declared ({lengths[b]})')
        if e < pushed:
            raise ValueError(f'stream {b}: length {e} lies before this chunk ({unit} {pushed} .. {pushed + n}): '
                             f'its {unit} were already emitted unmasked; declare the end with the chunk it lies in')
        if e > pushed + n:
            raise ValueError(f'stream {b}: length {e} lies beyond this chunk ({unit} {pushed} .. {pushed + n})')
        new[b] = e
    return new


def audio_chunk_bound(max_chunk):
    """Most samples one ``push_audio`` call takes: 160 * (max_chunk - 8).  n samples
    complete at most n // 160 + 1 feature frames; the end of a stream releases the 4 frames
    its delta-delta held back; at most 3 frames wait for their group of 4: n // 160 + 8
    frames at the most, which one ``push`` of max_chunk frames must take."""
    return 160 * (int(max_chunk) - 8)


def check_audio_chunk(n, max_chunk):
    bound = audio_chunk_bound(max_chunk)
    if n > bound:
        raise ValueError(f'push_audio takes at most 160 * (max_chunk - 8) = {bound} samples per call '
                         f'(max_chunk = {max_chunk}), got {n}')


def resampled_chunk_bound(max_chunk, iu, ou, hold):
    """Most input samples one ``push_audio`` call takes through a resampler of ratio iu : ou
    that holds back at most ``hold`` outputs: n inputs release at most ceil(n ou / iu) + hold
    outputs (what n_out grows by, plus what the end of the streams lets go), which one
    ``FbankStream.push`` of audio_chunk_bound(max_chunk) samples must take."""
    return max(0, audio_chunk_bound(max_chunk) - int(hold)) * int(iu) // int(ou)


class StreamOut:
    """What one ``push`` / ``finish`` emitted: output frames [t0, t0 + m) of every
    stream.  ``logits`` [B, m, C] (device); ``labels``: per stream, the greedy labels
    these frames added; ``label_frames``: per stream, the global output frame at which
    each of those labels was emitted, the first frame of its arg-max run (both fetched
    from the device together, on first use).  From a router with an endpointer,
    ``segments``: per stream, the ``endpoint.Segment``s this step closed (fetched with the
    labels)."""

    def __init__(self, router, t0, logits):
        self._router, self.t0, self.logits, self._labels, self._frames = router, t0, logits, None, None
        self._segments = None

    @property
    def segments(self):
        if self._router._ep is None:
            raise ValueError('this router does not segment its streams: build it with endpoint=EndpointRules(...)')
        if self._segments is None:
            self._router._fetch_labels()
        return [list(s) for s in self._segments]

    @property
    def labels(self):
        if self._labels is None:
            self._router._fetch_labels()
        return self._labels

    @property
    def label_frames(self):
        if self._frames is None:
            self._router._fetch_labels()
        return self._frames


class StreamingRouter:
    """``n_streams`` utterances through ``model`` (evaluation mode; naive or lowmemory,
    DR or SDR) in lock step, in chunks of at most ``max_chunk`` input frames.

    ``push(feats, ended=None)`` / ``finish()`` return a ``StreamOut``; ``reset()`` starts
    over; ``lookahead`` is 2 + L * rpad output frames; ``hypotheses`` the greedy labels so
    far.  With ``beam_width`` (1 .. 128) every chunk's logits also extend a device beam
    search (ctc.BeamState, at most ``max_frames`` output frames per stream, 4096 by
    default): ``beam_hypotheses`` and ``beam_scores`` are its result so far; with ``lm`` (a
    ``srf_amd.lm.FusedLM``) that language model is fused into the beam and the scores are
    the fused ones.  The model's parameters and BatchNorm moving statistics are read, never
    written.

    With ``frontend`` (a ``srf_amd.fbank.Fbank``) the router also takes audio:
    ``push_audio(samples [B, n], ended=None)`` extracts the features of the next n samples
    of every stream (``fbank.FbankStream``), holds the final feature frames back to a
    multiple of 4 and hands them to ``push``; ``ended`` is the sample-domain one (a stream's
    total sample count if its end lies in this chunk, else -1), from which the frame-domain
    one is derived.  The returned ``StreamOut`` is empty when no group of 4 frames became
    final.  One call takes at most ``audio_chunk_bound(max_chunk)`` = 160 * (max_chunk - 8)
    samples, so that one ``push`` of at most max_chunk frames takes what it completes, the
    end-of-stream flush included; more raises ``ValueError``.  ``finish()`` flushes the front
    end first, ``reset()`` resets it.  ``lookahead_audio_ms`` is what the audio side adds to
    the model's lookahead: 4 feature frames (the delta-delta's reach, 40 ms) plus the
    frame's own 25 ms.  A front end whose CMVN is a ``fbank.SlidingCmvn`` normalises online
    and adds nothing to that; ``reset(carry_cmvn=True)`` keeps what it learnt about each
    stream's speaker as the prior of the next utterance.

    With ``resampler`` as well (a single-rate ``srf_amd.resample.Resampler`` whose output rate
    is 16 kHz) ``push_audio`` takes samples at the resampler's input rate, ``ended`` in input
    samples, and feeds ``resample.ResampleStream`` -> ``FbankStream`` -> ``push``.  One call
    then takes at most ``audio_bound`` input samples, the largest chunk whose outputs cannot
    exceed audio_chunk_bound(max_chunk); ``lookahead_audio_ms`` grows by the filter's half
    width, 6000 / (0.99 min(fin, fout)) ms.

    With ``endpoint`` (an ``srf_amd.endpoint.EndpointRules``) the
    decoders are segmented per stream, on the device, with no host synchronisation in the
    chunk step: every step's logits go through an ``endpoint.Endpointer``, and where it
    closes a stream's segment the beam search of that stream alone starts over
    (``ctc.BeamState.push_cut``).  ``segments`` (and ``StreamOut.segments`` for one step)
    are, per stream, the ``endpoint.Segment``s closed so far: bounds, reason, the greedy
    labels whose emission frame (``label_frames``) lies in [start, end] -- a label run that
    crosses a forced cut belongs to the earlier segment, the one its first frame lies in --
    and the beam's best prefix of the segment with its score.  ``finish()`` closes every
    stream's open remainder as a last segment with reason 0.  ``beam_hypotheses`` is then the
    open segment's hypothesis, ``hypotheses`` stays the whole stream's.  The model is not
    restarted, so a stream may run without an end: the forced cut at ``max_segment`` frames
    bounds the beam's trie, and ``max_frames`` need only be max_segment + the most output
    frames one step emits.  The rules' smallest count must be at least that many frames, so
    that at most one cut per stream falls into a step.  What does grow with the stream are
    the host lists behind ``segments`` and ``hypotheses`` (and the steps' device results
    until something is fetched): ``pop_segments()`` hands the closed segments over and drops
    them and their labels."""

    def __init__(self, model, n_streams, max_chunk=64, beam_width=None, max_frames=None, lm=None, frontend=None,
                 resampler=None, endpoint=None):
        if model.caps_type == 'einsum':
            raise ValueError('the einsum variant cannot stream: its positional encoding needs the absolute frame '
                             'index, which srf_primary_caps_fwd_ex does not take')
        if model.pose_fp8:
            raise ValueError('model_pose_fp8 is not supported by the streaming path')
        if int(n_streams) < 1:
            raise ValueError(f'n_streams must be >= 1, got {n_streams}')
        if int(max_chunk) < 4 or int(max_chunk) % 4:
            raise ValueError(f'max_chunk must be a positive multiple of 4 input frames, got {max_chunk}')
        if lm is not None and not beam_width:
            raise ValueError('lm is fused into the beam search: it comes with a beam_width')
        self.model, self.B, self.max_chunk = model, int(n_streams), int(max_chunk)
        self.L, self.lpad, self.rpad = model.enc_num, model.lpad, model.rpad
        self.lookahead = 2 + self.L * self.rpad
        # audio side: a feature frame is final 4 frames (10 ms each) after its own 25 ms
        self.lookahead_audio_ms = 4 * 10 + 25 if frontend is not None else 0
        self._fe = None
        if frontend is not None:
            from . import fbank
            if model.feat_dim_in != fbank.N_FEAT:
                raise ValueError(f'the front end makes {fbank.N_FEAT}-d features, the model reads {model.feat_dim_in}')
            if audio_chunk_bound(max_chunk) < 1:
                raise ValueError(f'a front end needs max_chunk >= 12 input frames, got {max_chunk}')
            self._fe = fbank.FbankStream(frontend, int(n_streams), audio_chunk_bound(max_chunk))
        self._rs = None
        if resampler is not None:
            from . import resample
            if frontend is None:
                raise ValueError('a resampler feeds the front end: it comes with a frontend')
            if resampler.rate_out != 16000:
                raise ValueError(f'the front end reads 16 kHz audio, the resampler makes {resampler.rate_out} Hz')
            f = resampler.filters[0]
            hold = resample.stream_hold(f['first'], f['taps'], f['iu'])
            self.audio_bound = resampled_chunk_bound(max_chunk, f['iu'], f['ou'], hold)
            if self.audio_bound < 1:
                raise ValueError(f'max_chunk = {max_chunk} leaves no room for a chunk of resampled audio')
            self._rs = resample.ResampleStream(resampler, int(n_streams), self.audio_bound)
            self._audio_bound_why = (f'(160 * (max_chunk - 8) - {hold}) * {f["iu"]} // {f["ou"]} = {self.audio_bound} '
                                     f'samples at {resampler.rates_in[0]} Hz')
            self.lookahead_audio_ms += 6000.0 / (0.99 * min(resampler.rates_in[0], resampler.rate_out))
        self.blank = model.class_n - 1
        self.device = model.flat_params.device
        # the routing buffers' timeline: the last layer's next frame D sits at local
        # lpad + 1 (its window's left edge at 1, its SDR carry at lpad); the newest
        # primary-capsule frame is at most max_chunk / 4 + L * rpad frames ahead of D
        # (2 + L * rpad at finish), and an SDR pose at finish reads rpad zero frames more
        self.cap = self.max_chunk // 4 + (self.L + 1) * self.rpad + self.lpad + 3
        # with a beam width: the device prefix beam search next to the greedy decoder, its
        # beams carried from chunk to chunk (at most max_frames output frames per stream)
        self._beam = None
        max_frames = 4096 if max_frames is None else int(max_frames)
        # with an endpointer: the decoders are cut into segments per stream; at most one cut
        # per stream and step, since after a cut sil and n restart at 0 and speech is false
        # again, so the next cut needs min(counts) further frames and a step emits at most nmax
        self._ep = None
        if endpoint is not None:
            from . import endpoint as ep
            if not isinstance(endpoint, ep.EndpointRules):
                raise ValueError(f'endpoint must be an EndpointRules, got {type(endpoint).__name__}')
            nmax = max(self.max_chunk // 4, self.lookahead)
            if min(endpoint.counts) < nmax:
                raise ValueError(f'one step emits up to max(max_chunk // 4, lookahead) = {nmax} output frames: every '
                                 f'count of the endpoint rules must be at least that, so that at most one cut per '
                                 f'stream falls into a step; got {endpoint!r}')
            if beam_width and max_frames < endpoint.max_segment + nmax:
                raise ValueError(f'a segment takes up to max_segment = {endpoint.max_segment} output frames and a step '
                                 f'up to {nmax} more: the beam search needs max_frames >= '
                                 f'{endpoint.max_segment + nmax}, got {max_frames}')
            self._ep = ep.Endpointer(endpoint, self.B, model.class_n, self.blank, self.device)
            self._seg_max_len = endpoint.max_segment   # a segment's prefix has at most a label per frame
        if beam_width:
            self._beam = ctc.BeamState(self.B, model.class_n, self.blank, beam_width, max_frames, self.device, lm=lm,
                                       segmented=endpoint is not None)
        self._alloc()
        self.reset()

    # ------------------------------------------------------------------ state
    def _alloc(self):
        m, B, dev = self.model, self.B, self.device
        f32 = dict(device=dev, dtype=torch.float32)
        self._emb, self._v, self._u, self._ws = [], [], [], []
        nmax = max(self.max_chunk // 4, self.lookahead)   # frames one call makes final per layer
        for l, (in_n, J, D, din) in enumerate(m.layer_shapes):
            self._emb.append(torch.zeros((B, self.cap, in_n // m.window, din), **f32))
            if m.is_context:
                self._v.append(torch.zeros((B, self.cap, J, D), **f32))
                self._u.append(torch.empty(B * nmax * in_n * J * D, **f32))
                self._ws.append(self._recur_workspace(in_n, J, D))
        self._tail = torch.zeros((B, 4, m.feat_dim_in), **f32)
        self._len_dev = torch.full((B,), _NO_END, device=dev, dtype=torch.int32)
        self._prev = torch.full((B,), -1, device=dev, dtype=torch.int32)

    def _recur_workspace(self, in_n, J, D):
        n = _lib.lib().srf_route_sdr_recur_workspace(self.B, in_n, J, D, self.model.route_iters)
        return torch.zeros(max(n, 16), device=self.device, dtype=torch.uint8)

    def reset(self, carry_cmvn=False):
        """Every stream back at its start.  ``carry_cmvn``: a front end with a sliding CMVN
        keeps what it learnt about each stream's speaker as the prior of the next utterance
        (``fbank.FbankStream.reset(carry=True)``)."""
        if carry_cmvn and self._fe is None:
            raise ValueError('carry_cmvn needs a front end with a sliding CMVN')
        for t in self._emb + self._v:
            t.zero_()   # zero frames before the start: the window's padding and the SDR carry v_0 = 0
        self._tail.zero_()
        self._len_dev.fill_(_NO_END)
        self._prev.fill_(-1)
        self._x = None          # CNN-FE frames [_xg, ...) the primary capsules still need
        self._xg = 0
        self._base = -(self.lpad + 1)
        self._pushed = 0
        self._lengths = [None] * self.B
        self._finished = False
        self._hyp = [[] for _ in range(self.B)]
        self._hyp_frames = [[] for _ in range(self.B)]
        self._pending = []      # (StreamOut, labels, frames, count, cuts) not yet fetched from the device
        self._segs = [[] for _ in range(self.B)]   # with an endpointer: the segments closed so far
        self._seg_from = [0] * self.B              # labels of _hyp that belong to closed segments
        self._seg_open = [0] * self.B              # first frame of each stream's open segment
        if self._ep is not None:
            self._ep.reset()
        if self._beam is not None:
            self._beam.reset()
        self._beam_best = None  # (labels, scores) of the frames pushed so far, once fetched
        if self._fe is not None:
            self._fe.reset(carry=carry_cmvn)
        if self._rs is not None:
            self._rs.reset()
        self._held = None       # final feature frames that wait for their group of 4
        self._frame_len = [None] * self.B   # frame counts of the streams whose audio ended

    def _fetch_beam(self):
        if self._beam is None:
            raise ValueError('this router decodes greedily only: build it with a beam_width')
        if self._beam_best is None:
            self._beam_best = self._beam.best()
        return self._beam_best

    @property
    def beam_hypotheses(self):
        """Per stream, the beam search's most probable labelling of the frames emitted so
        far (beam_search_decode at the width given; fetched from the device on first use)."""
        return [list(h) for h in self._fetch_beam()[0]]

    @property
    def beam_scores(self):
        """Per stream, the log probability of its beam hypothesis (numpy)."""
        return self._fetch_beam()[1].copy()

    @property
    def hypotheses(self):
        """Per stream, the greedy labels of the frames emitted so far (frames below
        ceil(len / 4))."""
        self._fetch_labels()
        return [list(h) for h in self._hyp]

    @property
    def hypothesis_frames(self):
        """Per stream, the global output frame at which each label of ``hypotheses`` was
        emitted (an output frame is 4 input frames)."""
        self._fetch_labels()
        return [list(f) for f in self._hyp_frames]

    @property
    def segments(self):
        """Per stream, the ``endpoint.Segment``s closed so far (fetched with the labels)."""
        if self._ep is None:
            raise ValueError('this router does not segment its streams: build it with endpoint=EndpointRules(...)')
        self._fetch_labels()
        return [list(s) for s in self._segs]

    def pop_segments(self):
        """``segments``, handed over: the closed segments are returned and forgotten, and
        their greedy labels leave ``hypotheses`` / ``hypothesis_frames``, which from then on
        hold the labels of the open segments alone.  The host lists otherwise grow with the
        stream, a label per emitted label; a router that runs without an end calls this (or
        reads every ``StreamOut``) now and then."""
        out = self.segments
        for b in range(self.B):
            del self._hyp[b][:self._seg_from[b]], self._hyp_frames[b][:self._seg_from[b]]
        self._segs = [[] for _ in range(self.B)]
        self._seg_from = [0] * self.B
        return out

    def _fetch_labels(self):
        for out, labels, frames, count, cuts in self._pending:
            labels, frames, count = labels.cpu().tolist(), frames.cpu().tolist(), count.cpu().tolist()
            out._labels = [labels[b][:count[b]] for b in range(self.B)]
            out._frames = [frames[b][:count[b]] for b in range(self.B)]
            for b in range(self.B):
                self._hyp[b].extend(out._labels[b])
                self._hyp_frames[b].extend(out._frames[b])
            if self._ep is not None:
                out._segments = self._closed(cuts)
        self._pending = []

    def _take_labels(self, b, end):
        """The greedy labels of stream b emitted up to frame ``end`` that no segment has yet."""
        lo = hi = self._seg_from[b]
        fr = self._hyp_frames[b]
        while hi < len(fr) and fr[hi] <= end:
            hi += 1
        self._seg_from[b] = hi
        return self._hyp[b][lo:hi]

    def _closed(self, cuts):
        """One step's cuts (device tensors) as per-stream lists of Segments, also appended to
        ``segments``.  Called once the step's greedy labels are in ``_hyp``."""
        bounds, beam = cuts
        new = [[] for _ in range(self.B)]
        if bounds is None:
            return new
        # [B][3]: start, end, reason of the step's one cut, -1 without
        bounds = torch.cat([bounds.start[:, :1], bounds.end[:, :1], bounds.reason[:, :1]], dim=1).cpu().tolist()
        if beam is not None:
            count = beam[1].cpu().tolist()
            labels = beam[0][:, :max(count + [1])].cpu().tolist()
            score = beam[2].cpu().double().tolist()
            lm_score = None if beam[3] is None else beam[3].cpu().double().tolist()
        from .endpoint import Segment
        for b, (start, end, reason) in enumerate(bounds):
            if end < 0:
                continue
            seg = Segment(start, end, reason, self._take_labels(b, end))
            if beam is not None:
                seg = seg._replace(beam_labels=labels[b][:count[b]], beam_score=score[b],
                                   lm_score=None if lm_score is None else lm_score[b])
            new[b].append(seg)
            self._segs[b].append(seg)
            self._seg_open[b] = end + 1
        return new

    def _close_open_segments(self, out):
        """At finish(): every stream's open remainder as its last segment, reason 0, from the
        beam's best()."""
        self._fetch_labels()
        from .endpoint import Segment
        beam = self._fetch_beam() if self._beam is not None else None
        lm_score = None
        if beam is not None and self._beam.lm is not None:
            lm_score = self._beam.best_device()[3].cpu().double().tolist()
        for b in range(self.B):
            total = (self._pushed if self._lengths[b] is None else self._lengths[b]) + 3
            start, end = self._seg_open[b], total // 4 - 1
            if end < start:
                continue   # the stream's last frame closed a segment: nothing is open
            seg = Segment(start, end, 0, self._take_labels(b, end))
            if beam is not None:
                seg = seg._replace(beam_labels=list(beam[0][b]), beam_score=float(beam[1][b]),
                                   lm_score=None if lm_score is None else lm_score[b])
            out._segments[b].append(seg)
            self._segs[b].append(seg)
            self._seg_open[b] = end + 1

    # ------------------------------------------------------------------ stages
    def _local_len(self, offset, frames):
        """Input-frame lengths relative to a buffer that starts at input frame ``offset``
        and spans ``frames`` of them; the buffer's length while the end is unknown."""
        return (self._len_dev - offset).clamp_(0, frames)

    def _cnnfe(self, buf, lens):
        m = self.model
        moving = [getattr(m, n) for n in ('bn0_moving_mean', 'bn0_moving_var', 'bn1_moving_mean', 'bn1_moving_var')]
        return ops.cnnfe(buf, lens, [m.P(k) for k in ops.CNNFE_PARAMS], moving, False, 0.0, 0)

    def _caps(self, x, lens):
        m = self.model
        return ops.primary_caps(x, lens, m.caps_inp_n, m.caps_inp_d, False, 0.0, 0.0, 0,
                                [m.P(k) for k in ops.CAPS_PARAMS], m.proj_scale, False)

    def _dr(self, l, x):
        """DR layer l on the buffer slice x [B, Tx, N, din] -> v [B, Tx, J, D]."""
        m = self.model
        W, bias = m._identity.get(l, (m.P(f'W{l}'), m.P(f'b{l}')))
        return ops.dynamic_routing(x, W, bias, m._geom(l, self.B, x.shape[1]))

    def _norm(self, l, v):
        m = self.model
        return ops.CapsNorm.apply(v, m.P(f'ln_mid{l + 1}_gamma'), m.P(f'ln_mid{l + 1}_beta'), False, 0.0, 0, l)

    def _head(self, v):
        m, l = self.model, self.L - 1
        return ops.CapsHead.apply(v, m.P(f'ln_mid{l + 1}_gamma'), m.P(f'ln_mid{l + 1}_beta'),
                                  m.P('ln_output_gamma'), m.P('ln_output_beta'), False, 0.0, 0, l, m.length_eps)

    def _sdr(self, l, t0, t1):
        """SDR layer l over local frames [t0, t1): pose, the recurrence seeded from
        v[t0 - 1], and (inner layers) LayerNorm into the next layer's buffer.  The
        arguments are those of ops.SdrStack.forward's item()."""
        m, B, T = self.model, self.B, self.cap
        in_n, J, D, din = m.layer_shapes[l]
        L_ = _lib.lib()
        r = ops._sdr_r(t0=t0, t1=t1, emb=ops._ptr(self._emb[l]), W=ops._ptr(m.P(f'W{l}')), bias=ops._ptr(m.P(f'b{l}')),
                       u=ops._ptr(self._u[l]), v0=t0, vn=t1 - t0, v=ops._ptr(self._v[l]), couplings=None,
                       workspace=ops._ptr(self._ws[l]), workspace_bytes=self._ws[l].numel(), u_bf16=0, group=1)
        st = ops._stream()
        ops._sdr_call(L_.srf_route_sdr_pose_n, [r], B, T, in_n // m.window, din, m.lpad, m.rpad, J, D, 0, st,
                      what='sdr_pose_n')
        ops._sdr_call(L_.srf_route_sdr_recur_fwd_n, [r], B, T, in_n, J, D, m.route_iters, int(l == self.L - 1), st,
                      what='sdr_recur_fwd_n')
        if l < self.L - 1:
            cn = _lib.CapsnormRange(t0=t0, t1=t1, layer=l, x=ops._ptr(self._v[l]),
                                    gamma=ops._ptr(m.P(f'ln_mid{l + 1}_gamma')),
                                    beta=ops._ptr(m.P(f'ln_mid{l + 1}_beta')), y=ops._ptr(self._emb[l + 1]),
                                    stat=ops._ptr(self._stat(B * T)))
            ops._cn_call(L_.srf_capsnorm_fwd_range_n, [cn], B, T, J * D, 0, 0.0, 0, st, what='capsnorm_fwd_range_n')

    def _stat(self, rows):
        s = getattr(self, '_stat_buf', None)
        if s is None or s.shape[0] < rows:
            s = self._stat_buf = torch.empty((rows, 4), device=self.device, dtype=torch.float32)
        return s

    def _advance(self, shift, keep):
        ops.stream_advance([(t, self.cap, shift, keep) for t in self._emb + self._v])

    def _greedy(self, logits, n_valid, t0):
        return ctc.greedy_decode_frames_device(logits, n_valid, self.blank, self._prev, t0)

    # ------------------------------------------------------------------ the chunk step
    def push(self, feats, ended=None):
        """feats [B, n, feat_dim], n a multiple of 4 and at most max_chunk.  ``ended``
        [B]: the total input length of a stream whose end lies in this chunk, else -1."""
        if self._finished:
            raise ValueError('push after finish(): call reset() to start new utterances')
        if feats.dim() != 3 or feats.shape[0] != self.B or feats.shape[2] != self.model.feat_dim_in:
            raise ValueError(f'feats must be [{self.B}, n, {self.model.feat_dim_in}], got {tuple(feats.shape)}')
        n = feats.shape[1]
        if n % 4 or n > self.max_chunk:
            raise ValueError(f'a chunk holds a multiple of 4 input frames, at most max_chunk = {self.max_chunk}; '
                             f'got {n}')
        lengths = check_ended(self._lengths, ended, self._pushed, n)
        self._check_beam_room(n, False)
        if lengths != self._lengths:
            self._lengths = lengths
            self._len_dev.copy_(torch.tensor([_NO_END if e is None else e for e in lengths], dtype=torch.int32))
        with torch.no_grad():
            return self._step(feats.to(device=self.device, dtype=torch.float32), False)

    def push_audio(self, samples, ended=None):
        """samples [B, n] (int16 or float32, int16 scale), n <= audio_chunk_bound(max_chunk).
        ``ended`` [B]: the total sample count of a stream whose end lies in this chunk,
        else -1."""
        if self._fe is None:
            raise ValueError('this router takes features only: build it with a frontend')
        if self._finished:
            raise ValueError('push_audio after finish(): call reset() to start new utterances')
        if self._rs is not None:
            if samples.dim() == 2 and samples.shape[1] > self.audio_bound:
                raise ValueError(f'push_audio takes at most {self._audio_bound_why} per call '
                                 f'(max_chunk = {self.max_chunk}), got {samples.shape[1]}')
            with torch.no_grad():
                return self._push_frames(self._fe.push(*self._resampled(self._rs.push(samples, ended))), False)
        if samples.dim() == 2:
            check_audio_chunk(samples.shape[1], self.max_chunk)
        with torch.no_grad():
            return self._push_frames(self._fe.push(samples, ended), False)

    def _resampled(self, y):
        """(y, ended) for ``FbankStream.push``: the 16 kHz samples the resampler made final, with
        the output sample counts of the streams whose last output is among them."""
        rs, fe = self._rs, self._fe
        ended = [-1] * self.B
        for b, e in enumerate(rs.lengths):
            if e is not None and fe.lengths[b] is None and rs.rs.n_out(e) <= fe.pushed + y.shape[1]:
                ended[b] = rs.rs.n_out(e)
        return y, (ended if any(e >= 0 for e in ended) else None)

    def _push_frames(self, new, flush):
        """Final feature frames to ``push``, in groups of 4 (``flush``: all of them, zero
        padded to a group), with the ends of the streams whose last frame is among them."""
        from . import fbank
        fe = self._fe
        for b, e in enumerate(fe.lengths):
            if e is not None and self._frame_len[b] is None:
                self._frame_len[b] = fbank.n_frames(e)
        held = new if self._held is None else torch.cat([self._held, new], dim=1)
        flush = flush or all(e is not None for e in fe.lengths)
        n = held.shape[1] if flush else held.shape[1] // 4 * 4
        take, self._held = held[:, :n], held[:, n:]
        if n == 0:   # nothing for the model yet; an end at frame 0 is declared with the first group
            out = StreamOut(self, frames_final(self._pushed, self.L, self.rpad)[-1],
                            torch.empty((self.B, 0, self.model.class_n), device=self.device, dtype=torch.float32))
            out._labels, out._frames = [[] for _ in range(self.B)], [[] for _ in range(self.B)]
            out._segments = [[] for _ in range(self.B)]
            return out
        if n % 4:
            take = torch.cat([take, take.new_zeros((self.B, 4 - n % 4, take.shape[2]))], dim=1)
        # a stream's end is declared with the chunk its last frame lies in
        ended = [e if self._lengths[b] is None and e is not None and e <= self._pushed + take.shape[1] else -1
                 for b, e in enumerate(self._frame_len)]
        return self.push(take.contiguous(), ended if any(e >= 0 for e in ended) else None)

    def finish(self):
        """End of every stream: the frames still held back by the lookahead.  A stream
        that never declared a length ends with the last pushed frame.  With a front end,
        the feature frames it still holds go through ``push`` first, and the returned
        ``StreamOut`` covers both steps."""
        if self._finished:
            raise ValueError('finish() was already called: call reset() to start new utterances')
        first = []
        if self._fe is not None:
            with torch.no_grad():
                if self._rs is not None:
                    first.append(self._push_frames(self._fe.push(*self._resampled(self._rs.finish())), False))
                first.append(self._push_frames(self._fe.finish(), True))
        self._check_beam_room(0, True)
        with torch.no_grad():
            out = self._step(None, True)
        self._finished = True
        if self._ep is not None:
            self._close_open_segments(out)
        parts = [o for o in first if o.logits.shape[1]] + [out]
        if len(parts) > 1:
            self._fetch_labels()
            both = StreamOut(self, parts[0].t0, torch.cat([o.logits for o in parts], dim=1))
            both._labels = [sum((o._labels[b] for o in parts), []) for b in range(self.B)]
            both._frames = [sum((o._frames[b] for o in parts), []) for b in range(self.B)]
            if self._ep is not None:
                both._segments = [sum((o._segments[b] for o in parts), []) for b in range(self.B)]
            return both
        return out

    def _check_beam_room(self, n, finishing):
        """Refuse a step whose output frames the beam search cannot take, before anything
        advances: the router stays as it was, its hypotheses so far can be read, and
        reset() starts over.  (Not with an endpointer: its forced cut bounds the trie.)"""
        if self._beam is None or self._ep is not None:
            return
        emitted = frames_final(self._pushed + n, self.L, self.rpad, finished=finishing)[-1]
        if emitted > self._beam.shape[3]:
            raise ValueError(f'this step would bring the output frames to {emitted}, beyond the beam search\'s '
                             f'max_frames = {self._beam.shape[3]}: build the router with a larger max_frames')

    def _step(self, feats, finishing):
        B, lpad, rpad = self.B, self.lpad, self.rpad
        before = frames_final(self._pushed, self.L, rpad)
        n = 0 if finishing else feats.shape[1]
        P0, P1 = self._pushed, self._pushed + n
        after = frames_final(P1, self.L, rpad, finished=finishing)
        # CNN-FE on [4 kept | n new] (at finish: the kept frames alone, whose right edge is
        # the utterance's): the buffer starts at input frame P0 - 4, a multiple of 4, so
        # local output frame o is global frame P0 / 4 - 1 + o
        if after[0] > before[0]:
            buf = self._tail if finishing else torch.cat([self._tail, feats], dim=1)
            y = self._cnnfe(buf.contiguous(), self._local_len(P0 - 4, buf.shape[1]))
            lo = before[0] - (P0 // 4 - 1)
            new = y[:, lo:lo + after[0] - before[0]]
            self._x = new if self._x is None else torch.cat([self._x, new], dim=1)
        if n:
            self._tail = feats[:, -4:].clone()
        self._pushed = P1
        # primary capsules on the CNN-FE frames held: frame o needs frames o - 1 .. o + 1
        # (the kernel's zero padding of e is the reference's at the utterance's two ends)
        base = self._base
        if after[1] > before[1]:
            x = self._x.contiguous()
            z = self._caps(x, self._local_len(4 * self._xg, 4 * x.shape[1]))
            self._emb[0][:, before[1] - base:after[1] - base] = z[:, before[1] - self._xg:after[1] - self._xg]
            xg = max(0, after[1] - 1)
            self._x, self._xg = self._x[:, xg - self._xg:], xg
        # routing layers, bottom up: layer l's frames [a, b) are final once its input is
        # final up to b - 1 + rpad (at finish: up to the end, zero beyond it)
        logits = None
        for l in range(self.L):
            a, b, hi = before[l + 2], after[l + 2], after[l + 1]
            if b == a:
                continue
            t0, t1 = a - base, b - base
            if self.model.is_context:
                if finishing and rpad:
                    self._emb[l][:, hi - base:hi - base + rpad].zero_()
                self._sdr(l, t0, t1)
                v = self._v[l][:, t0:t1]
            else:
                # the window's halo (lpad + rpad frames) is routed again with every chunk
                v = self._dr(l, self._emb[l][:, t0 - lpad:min(t1 + rpad, hi - base)].contiguous())[:, lpad:lpad + b - a]
                if l < self.L - 1:
                    self._emb[l + 1][:, t0:t1] = self._norm(l, v.contiguous())
            if l == self.L - 1:
                logits = self._head(v.contiguous())
        t0, m = before[-1], after[-1] - before[-1]
        if logits is None:
            logits = torch.empty((B, 0, self.model.class_n), device=self.device, dtype=torch.float32)
        # slide the routing buffers: the last layer's next frame back to local lpad + 1
        new_base = after[-1] - lpad - 1
        if not finishing and new_base > base:
            self._advance(new_base - base, after[1] - new_base)
            self._base = new_base
        n_valid = ((self._len_dev + 3) // 4 - t0).clamp_(0, m).to(torch.int32)
        # with an endpointer: the segments this step's frames close (at most one per stream)
        bounds = self._ep.push(logits, n_valid, max_cuts=1) if self._ep is not None and m else None
        labels, frames, count = self._greedy(logits, n_valid, t0)
        closed = None
        if self._beam is not None:
            if bounds is None:
                self._beam.push(logits, n_valid)
            else:
                # a consuming stream has consumed t0 frames, so its cut's chunk frame is end - t0; -1 without a cut
                closed = self._beam.push_cut(logits, n_valid, (bounds.end[:, 0] - t0).clamp_(min=-1),
                                             max_len=self._seg_max_len)
            self._beam_best = None
        out = StreamOut(self, t0, logits)
        self._pending.append((out, labels, frames, count, (bounds, closed)))
        return out
