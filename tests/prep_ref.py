"""numpy statement of what the DR forward's operand preparation writes (route_fwd32.hip,
layouts above PrepArgs), din = dout = 32 with the split-fp16 backward operands.

    m = max|a|;  e = clamp(14 - frexp exponent of m, -60, 60), 0 for m = 0;  a' = a 2^e
    hi = float16(a') (round to nearest even),  lo = float16(float32(a') - float32(hi))

Every function returns the region's bytes as the kernel lays them out, so a test compares
them with `tobytes()`.
"""
import numpy as np


def split_exp(a):
    m = np.float32(np.abs(np.asarray(a, np.float32)).max()) if np.size(a) else np.float32(0)
    if not (m > 0) or not np.isfinite(m):
        return 0
    return int(max(-60, min(60, 14 - int(np.frexp(m)[1]))))


def split2h(a, e):
    s = (np.asarray(a, np.float32) * np.float32(2.0 ** e)).astype(np.float32)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def bf16_rne(a):
    """float32 -> bfloat16 bits (uint16), round to nearest even; finite inputs."""
    u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)


def bf16_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def regions(emb, W, bias, lpad, rpad, JDp):
    """emb [B][T][N][32], W [in_n][JD][32], bias [in_n][JD], all float32.  Returns the dict
    of regions Ws, bs, xs, WT, xT, hdr (numpy arrays in memory order) and aw, bx."""
    emb, W, bias = (np.ascontiguousarray(a, np.float32) for a in (emb, W, bias))
    B, T, N, D = emb.shape
    in_n, JD, _ = W.shape
    F, Fp = B * T, (B * T + 15) // 16 * 16
    aw, bx = split_exp(W), split_exp(emb)

    Ws = np.zeros((2, in_n, JDp, D), np.float16)
    Ws[0, :, :JD], Ws[1, :, :JD] = split2h(W, aw)

    b = (bias * np.float32(2.0 ** (aw + bx))).astype(np.float32)
    bs = np.zeros((in_n, JDp, 4), np.uint16)
    for k in range(3):
        bk = bf16_rne(b)
        bs[:, :JD, k] = bk
        b = (b - bf16_to_f32(bk)).astype(np.float32)

    x = emb.reshape(F, N, D)
    xs = np.zeros((2, N * F * D + 32), np.float16)   # capsule-major plane + the zero row
    hi, lo = split2h(x.transpose(1, 0, 2), bx)
    xs[0, :N * F * D], xs[1, :N * F * D] = hi.ravel(), lo.ravel()

    nt16 = (JD + 15) // 16
    Wp = np.zeros((2, in_n, nt16 * 16, D), np.float16)
    Wp[:, :, :JD] = Ws[:, :, :JD]
    # [plane][i][t][h][e][8 rows]
    WT = np.ascontiguousarray(Wp.reshape(2, in_n, nt16, 2, 8, D).transpose(0, 1, 2, 3, 5, 4))

    # window: capsule i = w N + n of frame (b, t) is emb[b][t + w - lpad][n], zero outside [0, T)
    nwin = lpad + rpad + 1
    xh, xl = split2h(emb, bx)
    win = np.zeros((2, nwin, N, Fp, D), np.float16)
    for w in range(nwin):
        t0, t1 = max(0, lpad - w), min(T, T + lpad - w)   # destination frames with a source row
        for p, src in enumerate((xh, xl)):
            dst = win[p, w, :, :F].reshape(N, B, T, D)
            dst[:, :, t0:t1] = src[:, t0 + w - lpad:t1 + w - lpad].transpose(2, 0, 1, 3)
    # [i][f / 16][plane][e][16 frames]
    xT = np.ascontiguousarray(win.reshape(2, nwin * N, Fp // 16, 16, D).transpose(1, 2, 0, 4, 3))

    hdr = np.array([2.0 ** -(aw + bx), aw, bx], np.float32)
    return {'Ws': Ws, 'bs': bs, 'xs': xs, 'WT': WT, 'xT': xT, 'hdr': hdr}, aw, bx


def xT_loop(emb, lpad, rpad, bx):
    """The xT region by a direct loop over (i, f, e): the check of regions()' indexing."""
    emb = np.asarray(emb, np.float32)
    B, T, N, D = emb.shape
    F, Fp = B * T, (B * T + 15) // 16 * 16
    nwin = lpad + rpad + 1
    out = np.zeros((nwin * N, Fp // 16, 2, D, 16), np.float16)
    for i in range(nwin * N):
        w, n = divmod(i, N)
        for f in range(F):
            b, t = divmod(f, T)
            ts = t + w - lpad
            if ts < 0 or ts >= T:
                continue
            for e in range(D):
                hi, lo = split2h(emb[b, ts, n, e], bx)
                out[i, f // 16, 0, e, f % 16] = hi
                out[i, f // 16, 1, e, f % 16] = lo
    return out
