"""The confidence-weighted edge-aware smoother (sm_wls_filter) in numpy float64: the executable
form of the definition in include/stereo_hip.h.  The fast global smoother of Min et al. (TIP 2014) used as OpenCV's
DisparityWLSFilter uses it: T passes of 1-D tridiagonal solves along every row, then every column, of the planes
N = confidence x disparity and M = confidence, whose links come from a guide image through a table of 256 weights; the
result is N / M.  Every operation below is one IEEE double operation, rounded on its own, in the order the header
writes it: the GPU path is held to these bits.

wls_filter is vectorised across the lines of a sweep and sequential along them; wls_filter_naive walks every line on
its own with Python floats (which are IEEE doubles): the two agree bit for bit (tests/test_wls_cpu.py).

WATCH: None, or a dict that every intermediate of wls_filter is reported to: {"tiny": the smallest non-zero magnitude
seen, "finite": all were finite}.  The tests use it to show that no pattern comes near a subnormal number."""
import numpy as np

NO_FILL = 1
WATCH = None


def _w(x):
    if WATCH is not None:
        nz = np.abs(x[x != 0])
        if nz.size:
            WATCH["tiny"] = min(WATCH.get("tiny", np.inf), float(nz.min()))
        WATCH["finite"] = WATCH.get("finite", True) and bool(np.isfinite(x).all())
    return x


def lambdas(lam, iterations):
    """lambda_t for t = 0 .. T - 1: ((1.5 lam) 4^(T-1-t)) / (4^T - 1.0), in double, in that order"""
    lam, T = float(lam), int(iterations)
    return [((1.5 * lam) * float(4 ** (T - 1 - t))) / (float(4 ** T) - 1.0) for t in range(T)]


def units(a):
    """the value in 1/16 steps as an exact double: 16 v for an int32 (web) map, v for an int16 (sub) map"""
    a = np.asarray(a)
    if a.dtype == np.int32:
        return 16.0 * a.astype(np.float64)
    if a.dtype == np.int16:
        return a.astype(np.float64)
    raise TypeError(f"need an int32 or int16 map, got {a.dtype}")


def start_planes(a, conf):
    """-> N = c u, M = c with c = (double)conf where a != 0, else 0"""
    a = np.asarray(a)
    c = np.full(a.shape, 255.0) if conf is None else np.asarray(conf).astype(np.float64)
    c = np.where(a != 0, c, 0.0)
    return c * units(a), c


def solve_lines(planes, links):
    """planes: arrays [m][n], each line of n elements solved on its own; links [m][n - 1] = l_0 .. l_(n-2) -> the solved
    planes.  The cp chain is computed once and serves every plane."""
    m, n = planes[0].shape
    if n == 1:
        return [p.copy() for p in planes]
    zero = np.zeros((m, 1))
    lp, ln = np.concatenate([zero, links], axis=1), np.concatenate([links, zero], axis=1)      # l_(i-1), l_i
    a, k, b = -lp, -ln, _w(_w(1.0 + lp) + ln)
    cp = np.empty((m, n))
    fp = [np.empty((m, n)) for _ in planes]
    inv = _w(1.0 / b[:, 0])
    cp[:, 0] = _w(k[:, 0] * inv)
    for f, p in zip(fp, planes):
        f[:, 0] = _w(p[:, 0] * inv)
    for i in range(1, n):
        den = _w(b[:, i] - _w(cp[:, i - 1] * a[:, i]))
        inv = _w(1.0 / den)
        cp[:, i] = _w(k[:, i] * inv)
        for f, p in zip(fp, planes):
            f[:, i] = _w(_w(p[:, i] - _w(f[:, i - 1] * a[:, i])) * inv)
    out = [np.empty((m, n)) for _ in planes]
    for u, f in zip(out, fp):
        u[:, n - 1] = f[:, n - 1]
        for i in range(n - 2, -1, -1):
            u[:, i] = _w(f[:, i] - _w(cp[:, i] * u[:, i + 1]))
    return out


def smooth_planes(N, M, guide, weights, lam, iterations):
    """the T passes over N and M (rows first, then columns) -> (N, M)"""
    g = np.asarray(guide).astype(np.int64)
    wd = np.asarray(weights).astype(np.float64)
    wrow, wcol = wd[np.abs(g[:, :-1] - g[:, 1:])], wd[np.abs(g[:-1, :] - g[1:, :])].T
    for lam_t in lambdas(lam, iterations):
        N, M = solve_lines([N, M], _w(lam_t * wrow))
        N, M = (p.T for p in solve_lines([np.ascontiguousarray(N.T), np.ascontiguousarray(M.T)], _w(lam_t * wcol)))
    return np.ascontiguousarray(N), np.ascontiguousarray(M)


def finish(a, N, M, flags, out_dtype):
    """-> (out, raw, filled)"""
    a = np.asarray(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = np.where(M > 0, N / np.where(M > 0, M, 1.0), 0.0)
    if flags & NO_FILL:
        raw = np.where(a != 0, raw, 0.0)
    out_dtype = np.dtype(out_dtype)
    info = np.iinfo(out_dtype)
    steps = np.rint(raw) if out_dtype == np.int16 else np.rint(raw / 16.0)
    out = np.clip(steps, float(info.min), float(info.max)).astype(out_dtype)
    return out, raw, int(((a == 0) & (out != 0)).sum())


def wls_filter(a, guide, weights, lam, iterations, conf=None, flags=0, out_dtype=None):
    """one map [H][W] -> (out [H][W] of out_dtype (default: a's), raw [H][W] float64, filled)"""
    a = np.asarray(a)
    N, M = start_planes(a, conf)
    N, M = smooth_planes(N, M, guide, weights, lam, iterations)
    return finish(a, N, M, flags, out_dtype or a.dtype)


# ---------------------------------------------------------------------------
# the same, line by line, in Python floats
# ---------------------------------------------------------------------------

def solve_line_naive(fs, links):
    """fs: lists of n floats (the planes of one line); links: n - 1 floats -> the solved lists"""
    n = len(fs[0])
    if n == 1:
        return [list(f) for f in fs]
    cp, fp = [0.0] * n, [[0.0] * n for _ in fs]
    for i in range(n):
        lp = links[i - 1] if i > 0 else 0.0
        ln = links[i] if i < n - 1 else 0.0
        a, k, b = -lp, -ln, (1.0 + lp) + ln
        den = b if i == 0 else b - cp[i - 1] * a
        inv = 1.0 / den
        cp[i] = k * inv
        for f, p in zip(fp, fs):
            f[i] = p[i] * inv if i == 0 else (p[i] - f[i - 1] * a) * inv
    out = [[0.0] * n for _ in fs]
    for u, f in zip(out, fp):
        u[n - 1] = f[n - 1]
        for i in range(n - 2, -1, -1):
            u[i] = f[i] - cp[i] * u[i + 1]
    return out


def wls_filter_naive(a, guide, weights, lam, iterations, conf=None, flags=0, out_dtype=None):
    a = np.asarray(a)
    h, w = a.shape
    g = [[int(v) for v in row] for row in np.asarray(guide)]
    wt = [float(v) for v in np.asarray(weights)]
    N, M = ([[float(v) for v in row] for row in p] for p in start_planes(a, conf))
    for lam_t in lambdas(lam, iterations):
        for y in range(h):
            N[y], M[y] = solve_line_naive([N[y], M[y]], [lam_t * wt[abs(g[y][x] - g[y][x + 1])] for x in range(w - 1)])
        for x in range(w):
            cn, cm = solve_line_naive([[N[y][x] for y in range(h)], [M[y][x] for y in range(h)]],
                                      [lam_t * wt[abs(g[y][x] - g[y + 1][x])] for y in range(h - 1)])
            for y in range(h):
                N[y][x], M[y][x] = cn[y], cm[y]
    return finish(a, np.array(N, np.float64).reshape(h, w), np.array(M, np.float64).reshape(h, w), flags, out_dtype or a.dtype)
