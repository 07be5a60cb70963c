"""Generate the committed fixtures under tests/golden/ -- TEST INFRASTRUCTURE ONLY.

Run in the build container (needs /root/reference for the flag fixtures):
    python -m oracle.gen_golden

* flags_*.json: argv -> parsed namespace produced by the REFERENCE parser
  (tfsr/helper/common_helper.py, TF-free, imported read-only from
  /root/reference).  The two .conf inputs are copied next to them as data.
* model_*.npz: SRF forward fixtures from the numpy float64 oracle
  (parity vs TF unpinned: TensorFlow is not installed), cross-checked at
  generation time against the float64 torch mirror; gradients from the mirror.
* model_*_eval.npz: the same models in evaluation mode (EVAL_CASES); regenerate
  some with ``python -m oracle.gen_golden c2_mini_eval c3_real_eval``.
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

from . import naive_mirror as nm
from . import srf_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
REF = '/root/reference'

FLAG_CASES = {
    # train_srf_timit.sh:45-65 with the script defaults overridden to BASELINE C2
    'timit_c2': ['--config=timit.conf', '--train-lr-param-k=0.5', '--train-batch-frame=7000',
                 '--train-warmup-n=1200', '--train-es-tolerance=27', '--train-max-epoch=27',
                 '--model-caps-primary-num=8', '--model-caps-convolution-num=8', '--model-caps-primary-dim=16',
                 '--model-caps-convolution-dim=16', '--model-caps-class-dim=16', '--model-caps-type=naive',
                 '--model-caps-window-lpad=4', '--model-caps-window-rpad=4', '--model-caps-context=false',
                 '--model-caps-iter=3', '--model-encoder-num=3'],
    # train_srf_wsj.sh:36-54 (BASELINE C3: SDR)
    'wsj_c3': ['--config=wsj.conf', '--train-lr-param-k=0.6', '--train-es-tolerance=15', '--train-max-epoch=15',
               '--model-caps-type=naive', '--model-caps-primary-num=16', '--model-caps-convolution-num=16',
               '--model-caps-primary-dim=32', '--model-caps-convolution-dim=32', '--model-caps-class-dim=32',
               '--model-caps-window-lpad=2', '--model-caps-window-rpad=2', '--model-caps-context=True',
               '--model-caps-iter=3', '--model-encoder-num=6'],
    'defaults_only': ['--model-caps-type=naive'],
    'buckets': ['--config=timit.conf', '--train-batch-buckets="[241, 391, 541]"', '--train-batch-dynamic=false',
                '--model-caps-context=no'],
}

MODEL_CASES = {
    # name: (SrfShape kwargs, B, lengths, label_len, seed)
    'c1_mini': (dict(feat_dim=123, enc_num=1, iters=1, lpad=0, rpad=0, ph=4, pd=8, ch=4, cd=8, vd=8,
                     class_n=63, context=False), 2, [41, 30], [6, 4], 11),
    'c2_mini': (dict(feat_dim=123, enc_num=3, iters=3, lpad=4, rpad=4, ph=8, pd=16, ch=8, cd=16, vd=16,
                     class_n=63, context=False), 2, [37, 29], [5, 3], 12),
    'c3_mini_sdr': (dict(feat_dim=123, enc_num=2, iters=3, lpad=2, rpad=2, ph=4, pd=8, ch=4, cd=8, vd=8,
                         class_n=32, context=True), 2, [26, 19], [4, 2], 13),
    # the other two reference variants (trainer_sr.py:188-199), C2-shaped but smaller
    'c2_mini_einsum': (dict(feat_dim=123, enc_num=2, iters=3, lpad=2, rpad=2, ph=8, pd=8, ch=8, cd=8, vd=8,
                            class_n=63, context=False, caps_type='einsum'), 2, [37, 29], [5, 3], 14),
    'c2_mini_lowmemory': (dict(feat_dim=123, enc_num=2, iters=3, lpad=2, rpad=2, ph=8, pd=8, ch=8, cd=8, vd=8,
                               class_n=63, context=False, caps_type='lowmemory'), 2, [37, 29], [5, 3], 15),
    'c3_mini_sdr_lowmemory': (dict(feat_dim=123, enc_num=2, iters=3, lpad=2, rpad=2, ph=4, pd=8, ch=4, cd=8, vd=8,
                                   class_n=32, context=True, caps_type='lowmemory'), 2, [26, 19], [4, 2], 16),
    # C4-shaped DR (DIM 32, WSJ classes): the din-32 split-fp16 routing path, with two
    # row tiles per wave in the inner layer (J*dout = 128) and four in the last (1024)
    'c4_mini': (dict(feat_dim=123, enc_num=2, iters=3, lpad=2, rpad=2, ph=4, pd=32, ch=4, cd=32, vd=32,
                     class_n=32, context=False), 2, [34, 27], [4, 3], 17),
}


# Full-size fixtures at BASELINE's real layer shapes.  Too large to
# store whole: feats are regenerated from a seed (float32-rounded, checksummed) and
# each parameter gradient is stored as a seeded sample of <= GRAD_SAMPLES entries
# plus its max |g| and L2 norm.
#   name: (SrfShape kwargs, lengths, label lengths, seed)
GRAD_SAMPLES = 4096
_C2 = dict(feat_dim=123, enc_num=3, iters=3, lpad=4, rpad=4, ph=8, pd=16, ch=8, cd=16, vd=16, class_n=63,
           context=False)
_WSJ = dict(feat_dim=123, enc_num=6, iters=3, lpad=2, rpad=2, ph=16, pd=32, ch=16, cd=32, vd=32, class_n=32)
BIG_CASES = {
    # C2 as bench.py runs it: B=17 utterances, the longest 320 frames (43 frame tiles x
    # 5 i-chunks on the last layer), the rest ragged inside the [241, 391) bucket
    'c2_full': (_C2, [320, 301, 288, 317, 249, 266, 310, 241, 295, 280, 319, 257, 270, 306, 244, 299, 262],
                None, 21),
    # C4 (DR) and C3 (SDR) at the true L=6, PH=CH=16, DIM=32, LPAD=RPAD=2 shapes
    'c4_real': (dict(_WSJ, context=False), [60, 47], [9, 6], 22),
    # SDR fixtures scale W (W_SCALE): at the reference's N(0, 0.1) init the deep SDR
    # recurrence is chaotic in fp32 -- a float32 run of the torch mirror differs from
    # the float64 oracle by 0.145 (C3) / 0.59 (C5) in the logits, and two float64
    # implementations by up to 0.79 at C5 -- so no fp32 implementation (TF's
    # included) can be held to 1e-4 there.  With W x 0.5 (C3) / x 0.25 (C5) the same
    # float32 mirror is within 1.9e-5 / 4.1e-6 of the oracle.
    'c3_real': (dict(_WSJ, context=True), [60, 47], [9, 6], 23),
    # C5: L=8, DIM=64, LPAD=RPAD=20 (in_n = 656), SDR with 5 iterations
    'c5_real': (dict(feat_dim=123, enc_num=8, iters=5, lpad=20, rpad=20, ph=16, pd=64, ch=16, cd=64, vd=64,
                     class_n=32, context=True), [40], [4], 24),
}
W_SCALE = {'c3_real': 0.5, 'c5_real': 0.25}


def scale_w(P, s):
    """W%d x s (the routing transforms only); shared with tests/helpers.py."""
    return {k: (v * s if k[0] == 'W' and k[1:].isdigit() else v) for k, v in P.items()}

# Data-parallel fixtures (world 2): one global batch of 4 ragged utterances split
# 2 + 2 as tf.distribute's rebatch does (restated below, independently of
# srf_amd.data_helper.split_global_batch); each
# replica crops to its own longest utterance (trainer_sr.py:59-60), normalises with its
# own batch statistics (Keras BN is not synchronised) and scales its loss by
# 1/(B_local * n_gpus) (trainer_sr.py:58,67-68).  The stored gradient is the SUM over
# replicas -- what the all-reduce in apply_gradients (trainer_sr.py:71) produces.
DP_CASES = {
    'dp2_c2_mini': (MODEL_CASES['c2_mini'][0], [37, 29, 33, 25], [5, 3, 4, 3], 31),
    'dp2_c4_mini': (MODEL_CASES['c4_mini'][0], [34, 27, 30, 22], [4, 3, 4, 2], 32),
}


def _labels(rng, tlens, class_n):
    labels = np.zeros((len(tlens), max(tlens)), dtype=np.int32)
    for b, l in enumerate(tlens):
        labels[b, :l] = rng.integers(1, class_n - 1, size=l)
    return labels


def regen_feats(seed, lens, feat_dim):
    """Synthetic N(0,1) fbank padded with zeros past each length (padded_batch,
    load_speech_data.py:151-156), float32-rounded; shared with tests/helpers.py."""
    rng = np.random.default_rng(seed + 100)
    feats = rng.standard_normal((len(lens), max(lens), feat_dim)).astype(np.float32).astype(np.float64)
    for b, l in enumerate(lens):
        feats[b, l:] = 0.0
    return feats


def _mirror_grads(sh, P, feats, inp_len, labels, tar_len, scale, tile):
    m = nm.NaiveMirror(sh, P, tile=tile)
    T = int(inp_len.max())
    lt = m(torch.tensor(feats[:, :T]), torch.tensor(inp_len))
    pe = nm.ctc_per_utt(lt, torch.tensor(labels), torch.tensor(inp_len), torch.tensor(tar_len), sh.class_n)
    (pe.sum() * scale).backward()
    grads = {k.replace('__', '.'): (p.grad.numpy() if p.grad is not None else np.zeros(p.shape))
             for k, p in m.p.items()}
    return lt.detach().numpy(), pe.detach().numpy(), grads


def _sampled(out, grads, seed):
    rng = np.random.default_rng(seed + 200)
    for k, g in grads.items():
        flat = g.reshape(-1)
        n = flat.size
        idx = np.arange(n) if n <= GRAD_SAMPLES else np.sort(rng.choice(n, GRAD_SAMPLES, replace=False))
        out['gidx.' + k] = idx.astype(np.int64)
        out['gval.' + k] = flat[idx].astype(np.float32)
        out['gstat.' + k] = np.array([np.abs(flat).max(), np.sqrt(np.square(flat).sum())])


def gen_big(only=()):
    for name, (kw, lens, tlens, seed) in BIG_CASES.items():
        if only and name not in only:
            continue
        sh = so.SrfShape(**kw)
        P = scale_w(so.init_params(sh, seed=seed), W_SCALE.get(name, 1.0))
        feats = regen_feats(seed, lens, sh.feat_dim)
        rng = np.random.default_rng(seed + 300)
        inp_len = np.array(lens, dtype=np.int32)
        if tlens is None:   # label lengths between T'/4 and T'/2 (bench: L = T'/2)
            tlens = [int(rng.integers(-(-l // 4) // 4, -(-l // 4) // 2 + 1)) for l in lens]
        tar_len = np.array(tlens, dtype=np.int32)
        labels = _labels(rng, tlens, sh.class_n)
        logits = so.srf_forward(P, sh, feats, inp_len)
        nll = so.ctc_batch(logits, labels, inp_len, tar_len, sh.class_n)
        greedy = so.greedy_decode(logits, np.ceil(inp_len / 4).astype(int), sh.class_n - 1)
        lt, pe, grads = _mirror_grads(sh, P, feats, inp_len, labels, tar_len, 1.0 / len(lens), tile=False)
        assert np.abs(lt - logits).max() < 1e-9, ('oracle/mirror disagree', np.abs(lt - logits).max())
        assert np.abs(pe - nll).max() < 1e-8, 'ctc oracle/torch disagree'
        srt = np.sort(logits, axis=-1)
        out = {'shape_json': np.array(json.dumps(kw)), 'feats_seed': np.array(seed),
               'feats_sum': np.array([feats.sum(), np.square(feats).sum()]), 'inp_len': inp_len, 'labels': labels,
               'tar_len': tar_len, 'logits': logits.astype(np.float32), 'nll': nll,
               'greedy_json': np.array(json.dumps(greedy)), 'seed': np.array(seed),
               'w_scale': np.array(W_SCALE.get(name, 1.0)),
               # smallest top-1 / top-2 logit gap over the valid frames (greedy decode margin)
               'greedy_margin': np.array(min(float((srt[b, :l, -1] - srt[b, :l, -2]).min())
                                             for b, l in enumerate(np.ceil(inp_len / 4).astype(int))))}
        out.update({'psum.' + k: np.array([v.sum(), np.square(v).sum()]) for k, v in P.items()})
        _sampled(out, grads, seed)
        np.savez_compressed(os.path.join(GOLD, f'model_{name}.npz'), **out)
        print(name, logits.shape, nll, 'margin', float(out['greedy_margin']))


# C3 at the reference's own initialisation (W ~ N(0, 0.1), naive:97-103, no W_SCALE):
# the float64 oracle's logits and NLL next to those of the float32 torch mirror (the
# same graph in fp32 on CPU), whose distance from the oracle is the chaos-amplified
# rounding any fp32 implementation carries there.  Gradients: seeded samples of both.
REFINIT_CASES = {'c3_refinit': (dict(_WSJ, context=True), [60, 47], [9, 6], 23)}

# C5 with the build's opt-in fp8 pose (BASELINE configs[4]): the float64 mirror with
# the pose replaced by srf_oracle.pose_fp8's declared quantisation (straight-through
# gradient), u in bf16 on the layers the library streams.  Same parameters / feats
# as c5_real (W x 0.25); the plain float64 oracle's logits sit in model_c5_real.npz.
FP8_CASES = {'c5_real_fp8': 'c5_real'}


def _c5_bf16_layers(sh):
    """Layers whose recurrence the library streams (srf_route_sdr_couplings_required):
    with the fp8 pose they keep u in bf16 (ops.SdrStackPlan.ubf)."""
    sys.path.insert(0, ROOT)
    from srf_amd import _lib
    L = _lib.lib()
    return [bool(L.srf_route_sdr_couplings_required(in_n, J, D, sh.route_iters))
            for (in_n, J, D, din) in sh.layer_shapes()]


REFINIT_PERTURB = 4


def gen_refinit(only=()):
    for name, (kw, lens, tlens, seed) in REFINIT_CASES.items():
        if only and name not in only:
            continue
        sh = so.SrfShape(**kw)
        P = so.init_params(sh, seed=seed)
        feats = regen_feats(seed, lens, sh.feat_dim)
        rng = np.random.default_rng(seed + 300)
        inp_len = np.array(lens, dtype=np.int32)
        tar_len = np.array(tlens, dtype=np.int32)
        labels = _labels(rng, tlens, sh.class_n)
        logits = so.srf_forward(P, sh, feats, inp_len)
        nll = so.ctc_batch(logits, labels, inp_len, tar_len, sh.class_n)
        _, _, g64 = _mirror_grads(sh, P, feats, inp_len, labels, tar_len, 1.0 / len(lens), tile=False)
        m = nm.NaiveMirror(sh, P, dtype=torch.float32, tile=False)
        T = int(inp_len.max())
        l32 = m(torch.tensor(feats[:, :T], dtype=torch.float32), torch.tensor(inp_len))
        pe32 = nm.ctc_per_utt(l32, torch.tensor(labels), torch.tensor(inp_len), torch.tensor(tar_len), sh.class_n)
        (pe32.sum() / len(lens)).backward()
        g32 = {k.replace('__', '.'): p.grad.double().numpy() for k, p in m.p.items()}
        # the spread of fp32 implementations: the same fp32 mirror on inputs whose last
        # mantissa bit is flipped at random (REFINIT_PERTURB runs)
        lp, np_, gp = [], [], []
        prng = np.random.default_rng(seed + 500)
        f32 = feats[:, :T].astype(np.float32)
        for _ in range(REFINIT_PERTURB):
            flip = prng.random(f32.shape) < 0.5
            fp = np.where(flip, np.nextafter(f32, np.where(prng.random(f32.shape) < 0.5, np.inf, -np.inf)
                                             .astype(np.float32)), f32).astype(np.float32)
            mk = nm.NaiveMirror(sh, P, dtype=torch.float32, tile=False)
            lk = mk(torch.tensor(fp), torch.tensor(inp_len))
            pk = nm.ctc_per_utt(lk, torch.tensor(labels), torch.tensor(inp_len), torch.tensor(tar_len), sh.class_n)
            (pk.sum() / len(lens)).backward()
            lp.append(lk.detach().numpy())
            np_.append(pk.detach().double().numpy())
            gp.append({k.replace('__', '.'): q.grad.double().numpy() for k, q in mk.p.items()})
        out = {'shape_json': np.array(json.dumps(kw)), 'feats_seed': np.array(seed),
               'feats_sum': np.array([feats.sum(), np.square(feats).sum()]), 'inp_len': inp_len, 'labels': labels,
               'tar_len': tar_len, 'logits': logits.astype(np.float32), 'nll': nll, 'seed': np.array(seed),
               'logits_m32': l32.detach().numpy(), 'nll_m32': pe32.detach().double().numpy(),
               'logits_m32p': np.stack(lp), 'nll_m32p': np.stack(np_)}
        out.update({'psum.' + k: np.array([v.sum(), np.square(v).sum()]) for k, v in P.items()})
        _sampled(out, g64, seed)
        for k, g in g32.items():
            out['gval32.' + k] = g.reshape(-1)[out['gidx.' + k]].astype(np.float32)
            out['gstat32.' + k] = np.array([np.abs(g).max(), np.sqrt(np.square(g).sum())])
            out['gval32p.' + k] = np.stack([gk[k].reshape(-1)[out['gidx.' + k]] for gk in gp]).astype(np.float32)
        np.savez_compressed(os.path.join(GOLD, f'model_{name}.npz'), **out)
        print(name, 'oracle vs fp32 mirror: logits', np.abs(l32.detach().numpy() - logits).max(),
              'nll', np.abs(pe32.detach().numpy() - nll).max(), 'perturbed runs:',
              [float(np.abs(x - logits).max()) for x in lp])


def gen_fp8(only=()):
    for name, base in FP8_CASES.items():
        if only and name not in only:
            continue
        kw, lens, tlens, seed = BIG_CASES[base]
        sh = so.SrfShape(**kw)
        P = scale_w(so.init_params(sh, seed=seed), W_SCALE.get(base, 1.0))
        feats = regen_feats(seed, lens, sh.feat_dim)
        rng = np.random.default_rng(seed + 300)
        inp_len = np.array(lens, dtype=np.int32)
        tar_len = np.array(tlens, dtype=np.int32)
        labels = _labels(rng, tlens, sh.class_n)
        bf = _c5_bf16_layers(sh)
        m = nm.NaiveMirror(sh, P, tile=False, fp8_pose=bf)
        T = int(inp_len.max())
        lt = m(torch.tensor(feats[:, :T]), torch.tensor(inp_len))
        pe = nm.ctc_per_utt(lt, torch.tensor(labels), torch.tensor(inp_len), torch.tensor(tar_len), sh.class_n)
        (pe.sum() / len(lens)).backward()
        grads = {k.replace('__', '.'): p.grad.numpy() for k, p in m.p.items()}
        logits = lt.detach().numpy()
        out = {'shape_json': np.array(json.dumps(kw)), 'feats_seed': np.array(seed), 'base': np.array(base),
               'feats_sum': np.array([feats.sum(), np.square(feats).sum()]), 'inp_len': inp_len, 'labels': labels,
               'tar_len': tar_len, 'logits': logits.astype(np.float32), 'nll': pe.detach().numpy(),
               'seed': np.array(seed), 'w_scale': np.array(W_SCALE.get(base, 1.0)),
               'bf16_layers': np.array(bf, dtype=np.int32)}
        out.update({'psum.' + k: np.array([v.sum(), np.square(v).sum()]) for k, v in P.items()})
        _sampled(out, grads, seed)
        np.savez_compressed(os.path.join(GOLD, f'model_{name}.npz'), **out)
        ref = np.load(os.path.join(GOLD, f'model_{base}.npz'))
        print(name, 'bf16 layers', bf, 'fp8-emulated vs fp64 oracle: logits',
              np.abs(logits - ref['logits']).max(), 'nll', out['nll'], ref['nll'])


def gen_dp(only=()):
    for name, (kw, lens, tlens, seed) in DP_CASES.items():
        if only and name not in only:
            continue
        sh = so.SrfShape(**kw)
        P = so.init_params(sh, seed=seed)
        feats = regen_feats(seed, lens, sh.feat_dim)
        rng = np.random.default_rng(seed + 300)
        inp_len = np.array(lens, dtype=np.int32)
        tar_len = np.array(tlens, dtype=np.int32)
        labels = _labels(rng, tlens, sh.class_n)
        world = 2
        total, nll = None, []
        B = len(lens)
        for rank in range(world):
            # rebatch: B // world each, the first B % world replicas one more, in order
            lo = rank * (B // world) + min(rank, B % world)
            hi = lo + B // world + (1 if rank < B % world else 0)
            f, lab, il, tl = feats[lo:hi], labels[lo:hi], inp_len[lo:hi], tar_len[lo:hi]
            _, pe, grads = _mirror_grads(sh, P, f, il, lab, tl, 1.0 / (len(il) * world), tile=True)
            nll.append(pe)
            total = grads if total is None else {k: total[k] + grads[k] for k in total}
        out = {'shape_json': np.array(json.dumps(kw)), 'feats_seed': np.array(seed),
               'feats_sum': np.array([feats.sum(), np.square(feats).sum()]), 'inp_len': inp_len, 'labels': labels,
               'tar_len': tar_len, 'nll': np.concatenate(nll), 'seed': np.array(seed), 'world': np.array(world)}
        out.update({'psum.' + k: np.array([v.sum(), np.square(v).sum()]) for k, v in P.items()})
        _sampled(out, total, seed)
        np.savez_compressed(os.path.join(GOLD, f'model_{name}.npz'), **out)
        print(name, out['nll'])


# Evaluation-mode fixtures (training=False: BatchNorm on its moving statistics, no
# dropout), model_<base>_eval.npz.  Parameters, feats, lengths and labels are the
# base fixture's ('base' names it; nothing of it is stored again).  The moving
# statistics are the oracle's batch mean / unbiased variance of an independently
# seeded batch (regen_feats(seed + 1000 + offset, [max(8, l - 5) ...])), rounded to
# float32: close to the data's own statistics, as in a trained model, not equal.
#   logits / nll: the oracle with bn_training=False (nll: ctc_batch, ceil lengths);
#   greedy_ceil_json / greedy_floor_json: best path at ceil(len/4) (validation) and
#     len // 4 (process_test_step, trainer_sr.py:110);
#   margin_ratio: min over the frames below the ceil length of
#     (top1 - top2) / (1e-4 (1 + max(|top1|, |top2|))) -- at >= EVAL_MARGIN no
#     implementation within the logit tolerance 1e-4 (1 + |ref|) can flip a label;
#   m32_err: max |m32 - o64| / (1 + |o64|) of the float32 torch mirror in eval mode,
#     required <= EVAL_M32 (half the GPU tolerance).
# 'offset' is the smallest of 0..15 meeting both conditions; none: an error.
EVAL_CASES = {n + '_eval': n for n in ('c1_mini', 'c2_mini', 'c3_mini_sdr', 'c2_mini_einsum', 'c2_mini_lowmemory',
                                       'c3_mini_sdr_lowmemory', 'c4_mini', 'c4_real', 'c3_real', 'c5_real',
                                       # the fp8-emulating float64 mirror in eval mode: 'logits' / 'nll'
                                       # are the emulation's, 'logits_o64' / 'nll_o64' the plain oracle's
                                       # on the same moving statistics; no m32 condition
                                       'c5_real_fp8')}
EVAL_MARGIN = 10.0
EVAL_M32 = 0.5e-4
EVAL_TOL = 1e-4


def margin_ratio(logits, lens):
    """Smallest top-1 / top-2 gap over the frames below ``lens``, in units of the
    logit tolerance EVAL_TOL (1 + max(|top1|, |top2|))."""
    r = np.inf
    for b, l in enumerate(lens):
        srt = np.sort(logits[b, :l], axis=-1)
        t1, t2 = srt[:, -1], srt[:, -2]
        r = min(r, float(((t1 - t2) / (EVAL_TOL * (1 + np.maximum(np.abs(t1), np.abs(t2))))).min()))
    return r


def eval_moving_stats(P, sh, seed, offset, lens):
    """{bn{k}.moving_mean / moving_var} (float32) from the independent batch."""
    lens2 = [max(8, l - 5) for l in lens]
    feats2 = regen_feats(seed + 1000 + offset, lens2, sh.feat_dim)
    _, stats = so.cnn_fe(P, sh, feats2, np.array(lens2, dtype=np.int32), bn_training=True)
    out = {}
    for k, (mu, var) in enumerate(stats):
        out[f'bn{k}.moving_mean'] = mu.astype(np.float32)
        out[f'bn{k}.moving_var'] = var.astype(np.float32)
    return out


def gen_eval(only=()):
    sys.path.insert(0, ROOT)
    from tests.helpers import load_model_fixture
    for name, base in EVAL_CASES.items():
        if only and name not in only:
            continue
        kw, sh, P, z = load_model_fixture(base)
        fp8 = base in FP8_CASES
        big = 'feats_seed' in z
        feats, inp_len, labels, tar_len = z['feats'], z['inp_len'], z['labels'], z['tar_len']
        lens = [int(l) for l in inp_len]
        ceil_len, floor_len = np.ceil(inp_len / 4).astype(int), (inp_len // 4).astype(int)
        T = int(inp_len.max())
        tf, tl = torch.tensor(feats[:, :T]), torch.tensor(inp_len)
        tried = []
        for offset in range(16):
            mv = eval_moving_stats(P, sh, int(z['seed']), offset, lens)
            Pe = dict(P, **{k: v.astype(np.float64) for k, v in mv.items()})
            o64 = so.srf_forward(Pe, sh, feats, inp_len, bn_training=False)
            extra = {}
            if fp8:
                bf = _c5_bf16_layers(sh)
                with torch.no_grad():
                    logits = nm.NaiveMirror(sh, Pe, tile=False, fp8_pose=bf)(tf, tl, bn_training=False).numpy()
                extra = {'logits_o64': o64.astype(np.float32),
                         'nll_o64': so.ctc_batch(o64, labels, inp_len, tar_len, sh.class_n),
                         'bf16_layers': np.array(bf, dtype=np.int32)}
            else:
                logits = o64
            ratio = margin_ratio(logits, ceil_len)
            if ratio < EVAL_MARGIN:
                tried.append((offset, 'margin', ratio))
                continue
            if not fp8:
                with torch.no_grad():
                    m64 = nm.NaiveMirror(sh, Pe, tile=not big)(tf, tl, bn_training=False).numpy()
                    m32 = nm.NaiveMirror(sh, Pe, dtype=torch.float32, tile=not big)(
                        tf.float(), tl, bn_training=False).double().numpy()
                assert np.abs(m64 - o64).max() < 1e-9, ('oracle/mirror disagree (eval)', np.abs(m64 - o64).max())
                m32_err = float((np.abs(m32 - o64) / (1 + np.abs(o64))).max())
                if m32_err > EVAL_M32:
                    tried.append((offset, 'm32', m32_err))
                    continue
                extra['m32_err'] = np.array(m32_err)
            break
        else:
            raise RuntimeError(f'{name}: no offset in 0..15 meets the conditions: {tried}')
        blank = sh.class_n - 1
        out = {'base': np.array(base), 'offset': np.array(offset),
               'logits': logits if not big else logits.astype(np.float32),
               'nll': so.ctc_batch(logits, labels, inp_len, tar_len, sh.class_n),
               'greedy_ceil_json': np.array(json.dumps(so.greedy_decode(logits, ceil_len, blank))),
               'greedy_floor_json': np.array(json.dumps(so.greedy_decode(logits, floor_len, blank))),
               'margin_ratio': np.array(ratio)}
        out.update(mv)
        out.update(extra)
        np.savez_compressed(os.path.join(GOLD, f'model_{name}.npz'), **out)
        print(name, 'offset', offset, 'rejected', tried, 'margin_ratio', ratio, 'm32_err',
              float(extra.get('m32_err', np.nan)), 'nll', out['nll'],
              'eval vs training-mode logits', float(np.abs(logits - z['logits']).max()))


def gen_flags():
    sys.path.insert(0, REF)
    from tfsr.helper.common_helper import Logger, ParseOption  # reference parser, read-only
    logger = Logger(name='golden', level=Logger.CRITICAL).logger
    for conf in ('timit.conf', 'wsj.conf'):
        shutil.copy(os.path.join(REF, 'egs', 'conf', conf), os.path.join(GOLD, conf))
    base = tempfile.mkdtemp()
    for name, argv in FLAG_CASES.items():
        full = ['prog', '--path-base=' + base] + [a.replace('--config=', '--config=' + GOLD + '/') for a in argv]
        args = vars(ParseOption(full, logger, is_print_opts=False).args)
        args['path_base'] = '<BASE>'
        if args.get('config'):
            args['config'] = os.path.basename(args['config'])
        with open(os.path.join(GOLD, f'flags_{name}.json'), 'w') as fh:
            json.dump({'argv': argv, 'parsed': args}, fh, indent=1, sort_keys=True)


def gen_models(only=()):
    for name, (kw, B, lens, tlens, seed) in MODEL_CASES.items():
        if only and name not in only:
            continue
        sh = so.SrfShape(**kw)
        P = so.init_params(sh, seed=seed)
        rng = np.random.default_rng(seed + 100)
        T = max(lens)
        feats = rng.standard_normal((B, T, sh.feat_dim))
        for b, l in enumerate(lens):
            feats[b, l:] = 0.0   # padded_batch zero padding (load_speech_data.py:151-156)
        inp_len = np.array(lens, dtype=np.int32)
        tar_len = np.array(tlens, dtype=np.int32)
        L = max(tlens)
        labels = np.zeros((B, L), dtype=np.int32)
        for b, l in enumerate(tlens):
            labels[b, :l] = rng.integers(1, sh.class_n - 1, size=l)
        logits = so.srf_forward(P, sh, feats, inp_len)
        nll = so.ctc_batch(logits, labels, inp_len, tar_len, sh.class_n)
        greedy = so.greedy_decode(logits, np.ceil(inp_len / 4).astype(int), sh.class_n - 1)
        # gradients of loss = sum(nll)/B from the float64 torch mirror
        m = nm.NaiveMirror(sh, P)
        lt = m(torch.tensor(feats), torch.tensor(inp_len))
        assert np.abs(lt.detach().numpy() - logits).max() < 1e-10, 'oracle/mirror disagree'
        pe = nm.ctc_per_utt(lt, torch.tensor(labels), torch.tensor(inp_len), torch.tensor(tar_len), sh.class_n)
        assert np.abs(pe.detach().numpy() - nll).max() < 1e-9, 'ctc oracle/torch disagree'
        (pe.sum() / B).backward()
        # no gradient (lowmemory DR W/b, unused by the graph): TF's apply_gradients skips them, stored as 0
        grads = {'grad.' + k.replace('__', '.'): (p.grad.numpy() if p.grad is not None else np.zeros(p.shape))
                 for k, p in m.p.items()}
        out = {'shape_json': np.array(json.dumps(kw)), 'feats': feats, 'inp_len': inp_len, 'labels': labels,
               'tar_len': tar_len, 'logits': logits, 'nll': nll,
               'greedy_json': np.array(json.dumps(greedy))}
        # parameters are regenerated from the seed by the tests (so.init_params);
        # per-parameter checksums pin that regeneration, gradients kept in fp32.
        out['seed'] = np.array(seed)
        out.update({'psum.' + k: np.array([v.sum(), np.square(v).sum()]) for k, v in P.items()})
        out.update({k: v.astype(np.float32) for k, v in grads.items()})
        np.savez_compressed(os.path.join(GOLD, f'model_{name}.npz'), **out)
        print(name, logits.shape, nll)


if __name__ == '__main__':
    os.makedirs(GOLD, exist_ok=True)
    only = sys.argv[1:]   # optional model case names: regenerate just those
    if not only:
        gen_flags()
    if not only or any(n in MODEL_CASES for n in only):
        gen_models([n for n in only if n in MODEL_CASES])
    if not only or any(n in BIG_CASES for n in only):
        gen_big([n for n in only if n in BIG_CASES])
    if not only or any(n in DP_CASES for n in only):
        gen_dp([n for n in only if n in DP_CASES])
    if not only or any(n in REFINIT_CASES for n in only):
        gen_refinit([n for n in only if n in REFINIT_CASES])
    if not only or any(n in FP8_CASES for n in only):
        gen_fp8([n for n in only if n in FP8_CASES])
    if not only or any(n in EVAL_CASES for n in only):   # last: they read their base fixtures
        gen_eval([n for n in only if n in EVAL_CASES])
