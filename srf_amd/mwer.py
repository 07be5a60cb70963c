"""Minimum word error rate (MWER) training on the device: the expected error of an N-best
list and its logit gradient (srf_mwer_loss; tfsr/helper/train_helper.py's loss_ewerr,
Prabhavalkar et al., ICASSP 2018).

The list comes from the device beam search (``ctc.BeamState.nbest``), its errors from the
device scoring kernels (``hypothesis_errors``), and ``mwer_loss_and_grad`` gives, per
utterance over its n listed hypotheses with errors e_i,

    p_i = P_CTC(y_i | x) / sum_k P_CTC(y_k | x),    loss = sum_i p_i (e_i - mean_k e_k),

with P_CTC the full sum over alignments (not the beam's score), and grad_scale * d loss /
d logits.  Nothing is copied to the host.
"""
import torch

from . import ops


def _ref_rows(ref, ref_len, B, N, dev):
    if not torch.is_tensor(ref) or ref.dim() != 2 or ref.shape[0] != B:
        raise ValueError(f'ref must be a tensor [{B}, Rmax], got {tuple(getattr(ref, "shape", ()))}')
    ref_len = torch.as_tensor(ref_len)
    if tuple(ref_len.shape) != (B,):
        raise ValueError(f'ref_len must have shape ({B},), got {tuple(ref_len.shape)}')
    r = ref.detach().to(device=dev, dtype=torch.int32)
    rl = ref_len.to(device=dev, dtype=torch.int32)
    return r.repeat_interleave(N, dim=0).contiguous(), rl.repeat_interleave(N).contiguous()


def hypothesis_errors(nbest, ref, ref_len, separator=None, fold=None):
    """The error count of every listed hypothesis against its utterance's reference, int32
    [B, N] on the device: word errors (srf_word_align) when ``separator`` (the label that
    parts words) is given, else label errors (srf_edit_align), labels folded through
    ``fold`` when given.  The list is scored as B * N rows, every reference row repeated N
    times; rows past the list's count score their reference's length and are not used."""
    from . import scoring
    B, N, Lmax = nbest.labels.shape
    dev = nbest.labels.device
    r, rl = _ref_rows(ref, ref_len, B, N, dev)
    h = nbest.labels.reshape(B * N, Lmax)
    hl = nbest.lengths.reshape(B * N)
    f = scoring._fold_tensor(fold, dev)
    if separator is not None:
        counts = ops.word_align(h, hl, r, rl, scoring._separator(separator), f, words=False, maps=False)[0]
    else:
        counts = ops.edit_align(h, hl, r, rl, f, maps=False)[0]
    return counts[:, 0].reshape(B, N).contiguous()


def _operands(logits, logit_len, nbest, errors):
    if not torch.is_tensor(logits) or logits.dim() != 3 or not logits.is_cuda:
        shape, where = tuple(getattr(logits, 'shape', ())), getattr(logits, 'device', 'the host')
        raise ValueError(f'logits must be a device tensor [B, T, C], got {shape} on {where}')
    dev = logits.device
    B = logits.shape[0]
    N = nbest.labels.shape[1]
    if nbest.labels.dim() != 3 or nbest.labels.shape[0] != B:
        raise ValueError(f'the N-best list holds {tuple(nbest.labels.shape)} labels for {B} utterances')
    if not 1 <= N <= 32:
        raise ValueError(f'the MWER loss takes lists of 1 .. 32 hypotheses, got {N}')

    def i32(t, shape, name):
        t = torch.as_tensor(t)
        if tuple(t.shape) != shape:
            raise ValueError(f'{name} must have shape {shape}, got {tuple(t.shape)}')
        return t.detach().to(device=dev, dtype=torch.int32).contiguous()
    return (i32(logit_len, (B,), 'logit_len'), i32(nbest.labels, tuple(nbest.labels.shape), 'labels'),
            i32(nbest.lengths, (B, N), 'lengths'), i32(nbest.count, (B,), 'count'), i32(errors, (B, N), 'errors'))


def mwer_loss_and_grad(logits, logit_len, nbest, errors, blank_index, grad_scale):
    """(loss [B], grad_scale * d(sum loss)/d logits [B, T, C], p_hat [B, N], hyp_logp
    [B, N]) from one call of srf_mwer_loss, without autograd.  ``nbest``: anything with
    ``labels`` [B, N, Lmax], ``lengths`` [B, N] and ``count`` [B] (``ctc.NBest``);
    ``errors`` int [B, N]."""
    ll, lab, ln, cnt, err = _operands(logits, logit_len, nbest, errors)
    return ops.mwer_loss_and_grad(logits.detach().float().contiguous(), ll, lab, ln, cnt, err, int(blank_index),
                                  float(grad_scale))


class MwerLoss(torch.autograd.Function):
    """Per-utterance expected error; the logit gradient comes out of the same call and is
    scaled by the incoming per-utterance gradient in backward."""

    @staticmethod
    def forward(ctx, logits, logit_len, lab, ln, cnt, err, blank):
        need_grad = logits.requires_grad
        loss, grad, _, _ = ops.mwer_loss_and_grad(logits.detach().float().contiguous(), logit_len, lab, ln, cnt, err,
                                                  blank, 1.0, want_grad=need_grad)
        if need_grad:
            ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        (grad,) = ctx.saved_tensors
        return grad * g_loss[:, None, None], None, None, None, None, None, None


def mwer_loss(logits, logit_len, nbest, errors, blank_index):
    """The expected error [B] of each utterance over its N-best list, differentiable in
    ``logits`` (the list and the errors are constants)."""
    ll, lab, ln, cnt, err = _operands(logits, logit_len, nbest, errors)
    return MwerLoss.apply(logits, ll, lab, ln, cnt, err, int(blank_index))
