"""Float64 reference and fp32 restatement of the exact enumeration (imdbn_rbm_exact_logz, kernels_exact.hpp).

E is the enumerated side (n units, bias e), S the other one (D units, bias f), Wd [n, D] the weights between them; state s has unit k
of E on iff bit k of s is set.  ``reference`` enumerates in float64 in chunks of states, so n = 23 on a narrow layer fits in memory;
``restate`` repeats the kernel's arithmetic: a fresh fp32 base every 32 states from the set bits k >= 5 in ascending order, the
Gray-code walk of the 5 low bits, the terms of S in fp32 inside chunks of 128 columns (two per lane) and in double across."""
import numpy as np

F32, F64 = np.float32, np.float64
LOG_2PI = float(np.log(2.0 * np.pi))


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def sides(W, b, c, side, groups=(), z=None):
    """(side name, e, f, Wd [n, D]) of the call: "auto" is the smaller side (ties: hidden), hidden with groups or Gaussian visibles."""
    V, H = W.shape
    if side == "auto":
        side = "hidden" if (z is not None or len(groups) > 0 or H <= V) else "visible"
    return (side, c, b, W.T) if side == "hidden" else (side, b, c, W)


def _free(D, groups):
    m = np.ones(D, bool)
    for s, e in groups:
        m[s:e] = False
    return m


def _bits(codes, n):
    return ((codes[:, None] >> np.arange(n)[None, :]) & 1).astype(F64)


def reference(W, b, c, side="auto", groups=(), z=None, marginals=False, chunk=1 << 16):
    """dict(log_z, log_w_max, side, bits, vis_mean, hid_mean, x_max), everything in float64.  ``x_max``: the largest |b_i + a_i| over
    all states (Gaussian visibles; the scale of the mean's tolerance)."""
    W, b, c = np.asarray(W, F64), np.asarray(b, F64), np.asarray(c, F64)
    side, e, f, Wd = sides(W, b, c, side, groups, z)
    assert side == "hidden" or (not groups and z is None)
    n, D = Wd.shape
    free = _free(D, groups)
    iv = None if z is None else np.exp(-np.asarray(z, F64))
    cz = 0.0 if z is None else float(0.5 * (LOG_2PI + np.asarray(z, F64)).sum())

    def weights(codes):
        st = _bits(codes, n)
        if z is not None:
            a = st @ Wd
            return st @ e + ((f * a + 0.5 * a * a) * iv).sum(1), f + a
        x = st @ Wd + f
        t = st @ e + softplus(x[:, free]).sum(1)
        for s0, e0 in groups:
            m = x[:, s0:e0].max(1)
            t = t + m + np.log(np.exp(x[:, s0:e0] - m[:, None]).sum(1))
        return t, x

    N = 1 << n
    mx, ssum = -np.inf, 0.0
    for lo in range(0, N, chunk):
        t, _ = weights(np.arange(lo, min(N, lo + chunk), dtype=np.int64))
        m2 = max(mx, float(t.max()))
        ssum = ssum * np.exp(mx - m2) + float(np.exp(t - m2).sum())
        mx = m2
    lse = mx + np.log(ssum)
    out = dict(log_z=lse + cz, log_w_max=mx + cz, side=side, bits=n, vis_mean=None, hid_mean=None, x_max=0.0)
    if not marginals:
        return out
    me, ms, xm = np.zeros(n), np.zeros(D), 0.0
    for lo in range(0, N, chunk):
        codes = np.arange(lo, min(N, lo + chunk), dtype=np.int64)
        t, x = weights(codes)
        w = np.exp(t - lse)
        me += w @ _bits(codes, n)
        if z is not None:
            ms += w @ x
            xm = max(xm, float(np.abs(x).max()))
        else:
            p = 1.0 / (1.0 + np.exp(-x))
            for s0, e0 in groups:
                g = np.exp(x[:, s0:e0] - x[:, s0:e0].max(1, keepdims=True))
                p[:, s0:e0] = g / g.sum(1, keepdims=True)
            ms += w @ p
    out["vis_mean"], out["hid_mean"] = (ms, me) if side == "hidden" else (me, ms)
    out["x_max"] = xm
    return out


def restate(W, b, c, side="auto", groups=(), z=None):
    """log Z as the kernel computes it (module docstring); the LSE over states in float64 (its order moves the result by ulps of a
    double).  Vectorised over the tiles of 32 states."""
    W32, b32, c32 = np.asarray(W, F32), np.asarray(b, F32), np.asarray(c, F32)
    side, e, f, Wd = sides(W32, b32, c32, side, groups, z)
    Wd = np.ascontiguousarray(Wd, F32)
    n, D = Wd.shape
    free = _free(D, groups)
    iv = None if z is None else np.exp(-np.asarray(z, F32)).astype(F32)
    n_tiles = max(1, (1 << n) >> 5)
    hi = np.arange(n_tiles, dtype=np.int64) << 5
    x = np.zeros((n_tiles, D), F32) if z is not None else np.broadcast_to(f, (n_tiles, D)).astype(F32)
    for k in range(5, n):
        on = ((hi >> k) & 1).astype(bool)
        x[on] = (x[on] + Wd[k][None, :]).astype(F32)
    tot = np.full((n_tiles, 32), -np.inf)
    lanes = np.arange(D) % 128 % 64 + 64 * (np.arange(D) // 128)      # (chunk, lane) of a column: the two columns of a lane add in fp32
    n_lane = int(lanes.max()) + 1
    e64 = np.asarray(e, F64)
    for t in range(32):
        code = t ^ (t >> 1)
        if t > 0:
            k = (t & -t).bit_length() - 1
            if k < n:
                x = (x + Wd[k][None, :]).astype(F32) if (code >> k) & 1 else (x - Wd[k][None, :]).astype(F32)
        if code >= (1 << n):
            continue
        if z is not None:
            term = ((f[None, :] * x + (F32(0.5) * x) * x) * iv[None, :]).astype(F32)
        else:
            ax = np.abs(x)
            term = (np.maximum(x, F32(0)) + np.log1p(np.exp(-ax).astype(F32)).astype(F32)).astype(F32)
            term[:, ~free] = 0
        pair = np.zeros((n_tiles, n_lane), F32)      # first column of the lane, then the second: one fp32 add
        first = (np.arange(D) % 128) < 64
        pair[:, lanes[first]] = term[:, first]
        second = np.zeros((n_tiles, n_lane), F32)
        second[:, lanes[~first]] = term[:, ~first]
        s = (pair + second).astype(F32).astype(F64).sum(1)
        for s0, e0 in groups:
            g = x[:, s0:e0]
            m = g.max(1)
            s = s + m.astype(F64) + np.log(np.exp((g - m[:, None]).astype(F32)).astype(F32).astype(F64).sum(1))
        codes = hi | code
        tot[:, code] = s + _bits(codes, n) @ e64
    t = tot.ravel()
    t = t[np.isfinite(t)]
    cz = 0.0 if z is None else float(0.5 * (LOG_2PI + np.asarray(z, F32).astype(F64)).sum())
    return float(t.max() + np.log(np.exp(t - t.max()).sum()) + cz)
