"""Independent numpy reference for the bulk RNG streams.

Re-implements, from the published algorithms, what cmb::Rng does for the
bulk kernels: fmix64 / splitmix64 / sfc64, the 53-bit uniforms and the
256-layer ziggurat for the standard normal and exponential.  Everything is
vectorised over lanes and steps one draw at a time with index masks; all
integer work is uint64 wrap-around arithmetic and the tables come from
`_C.zig_tables()` (the compiled constants), so the fast path is bit-exact
by construction and only `exp`/`log` can differ from the C++ code.

Layout (cimba/bulk_rng.hpp): lane g is seeded with
fmix64(seed ^ (g*0x9E3779B97F4A7C15 + 1)); sample i is draw i // lanes of
lane i % lanes.

Besides the samples, `generate` returns which samples came from the normal
tail (values that passed through `log`) and the smallest relative margin of
every accept/reject comparison that involved `exp` or `log`, evaluated in
np.longdouble: a margin far above the few-ulp spread between math libraries
proves that no implementation can take a different branch.

Plain module, imported by tests/test_rng_streams.py.
"""
from collections import namedtuple

import numpy as np

U = np.uint64
LD = np.longdouble
GOLDEN = U(0x9E3779B97F4A7C15)
TWO_M53 = 2.0 ** -53


def _u(x):
    return np.atleast_1d(np.asarray(x, dtype=U)).copy()


def fmix64(x):
    x = _u(x)
    x ^= x >> U(33)
    x *= U(0xFF51AFD7ED558CCD)
    x ^= x >> U(33)
    x *= U(0xC4CEB9FE1A85EC53)
    x ^= x >> U(33)
    return x


def splitmix64(state):
    """Advances `state` (uint64 array) in place, returns the outputs."""
    state += GOLDEN
    z = state.copy()
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def lane_seeds(seed, lanes):
    g = np.arange(lanes, dtype=U)
    return fmix64(U(seed) ^ (g * GOLDEN + U(1)))


class Sfc64:
    """One sfc64 stream per lane; every method takes the lane indices to
    advance and leaves the other lanes untouched."""

    def __init__(self, seeds):
        sm = _u(seeds)
        self.a = splitmix64(sm)
        self.b = splitmix64(sm)
        self.c = splitmix64(sm)
        self.counter = np.ones(sm.shape, dtype=U)
        every = np.arange(sm.size)
        for _ in range(12):
            self.next(every)

    def state(self):
        return self.a.copy(), self.b.copy(), self.c.copy(), self.counter.copy()

    def next(self, idx):
        a, b, c, k = self.a[idx], self.b[idx], self.c[idx], self.counter[idx]
        tmp = a + b + k
        self.counter[idx] = k + U(1)
        self.a[idx] = b ^ (b >> U(11))
        self.b[idx] = c + (c << U(3))
        self.c[idx] = ((c << U(24)) | (c >> U(40))) + tmp
        return tmp

    def u01(self, idx):
        return (self.next(idx) >> U(11)).astype(np.float64) * TWO_M53

    def u01_open(self, idx):
        return ((self.next(idx) >> U(11)).astype(np.float64) + 0.5) * TWO_M53


class Margin:
    """Smallest relative decision margin seen so far."""

    def __init__(self):
        self.min = np.inf

    def note(self, rel):
        if rel.size:
            self.min = min(self.min, float(rel.min()))


def std_exponential(rng, idx, T, margin):
    out = np.empty(idx.size)
    offset = np.zeros(idx.size)
    pend = np.arange(idx.size)  # positions in `out` still undecided
    X, F, RATIO, R = T["EXP_X"], T["EXP_F"], T["EXP_RATIO"], T["EXP_R"]
    while pend.size:
        lanes = idx[pend]
        r = rng.next(lanes)
        i = (r & U(255)).astype(np.intp)
        u = (r >> U(11)).astype(np.float64) * TWO_M53
        fast = u < RATIO[i]
        out[pend[fast]] = offset[pend[fast]] + u[fast] * X[i[fast]]
        tail = ~fast & (i == 0)
        offset[pend[tail]] += R
        w = ~fast & (i != 0)
        wi, wp = i[w], pend[w]
        x = u[w] * X[wi]
        lhs = F[wi + 1] + rng.u01(lanes[w]) * (F[wi] - F[wi + 1])
        fx = np.exp(-x)
        fx_ld = np.exp(-x.astype(LD))
        margin.note(np.abs(lhs.astype(LD) - fx_ld) / fx_ld)
        acc = lhs < fx
        out[wp[acc]] = offset[wp[acc]] + x[acc]
        pend = np.concatenate([pend[tail], wp[~acc]])
    return out


def std_normal(rng, idx, T, margin):
    """Returns (values, from_tail)."""
    out = np.empty(idx.size)
    from_tail = np.zeros(idx.size, dtype=bool)
    pend = np.arange(idx.size)
    X, F, RATIO, R = T["NOR_X"], T["NOR_F"], T["NOR_RATIO"], T["NOR_R"]
    while pend.size:
        lanes = idx[pend]
        r = rng.next(lanes)
        i = (r & U(255)).astype(np.intp)
        sign = np.where((r & U(256)) != 0, -1.0, 1.0)
        u = (r >> U(11)).astype(np.float64) * TWO_M53
        fast = u < RATIO[i]
        out[pend[fast]] = sign[fast] * u[fast] * X[i[fast]]

        # layer 0 beyond the rectangle: Marsaglia's tail, repeated until
        # 2y >= x^2; always ends with a sample
        t = ~fast & (i == 0)
        tp, tl, ts = pend[t], lanes[t], sign[t]
        while tp.size:
            u1 = rng.u01_open(tl)
            u2 = rng.u01_open(tl)
            x = -np.log(u1) / R
            y = -np.log(u2)
            x_ld = -np.log(u1.astype(LD)) / LD(R)
            y_ld = -np.log(u2.astype(LD))
            margin.note(np.abs(y_ld + y_ld - x_ld * x_ld) / (x_ld * x_ld))
            rej = y + y < x * x
            ok = ~rej
            out[tp[ok]] = ts[ok] * (R + x[ok])
            from_tail[tp[ok]] = True
            tp, tl, ts = tp[rej], tl[rej], ts[rej]

        w = ~fast & (i != 0)
        wi, wp = i[w], pend[w]
        x = u[w] * X[wi]
        arg = -0.5 * x * x  # double on every side; only exp() can differ
        fx = np.exp(arg)
        fx_ld = np.exp(arg.astype(LD))
        lhs = F[wi + 1] + rng.u01(lanes[w]) * (F[wi] - F[wi + 1])
        margin.note(np.abs(lhs.astype(LD) - fx_ld) / fx_ld)
        acc = lhs < fx
        out[wp[acc]] = sign[w][acc] * x[acc]
        pend = wp[~acc]
    return out, from_tail


def std_gamma(rng, idx, alpha, T, margin, dtype=np.float64):
    """Marsaglia-Tsang with the alpha<1 boost.  The normal deviate is the
    double stream above; the gamma arithmetic itself runs in `dtype`
    (np.float64 mirrors the C++ code, np.longdouble gives the same formula
    at higher precision) and the result is rounded to double."""
    f = dtype
    alpha = f(alpha)
    boost = np.ones(idx.size, dtype=f)
    if alpha < 1:
        boost = np.power(rng.u01_open(idx).astype(f), f(1) / alpha)
        alpha = alpha + f(1)
    d = alpha - f(1) / f(3)
    cc = f(1) / np.sqrt(f(9) * d)
    out = np.empty(idx.size)
    pend = np.arange(idx.size)
    while pend.size:
        x = np.empty(pend.size, dtype=f)
        v = np.empty(pend.size, dtype=f)
        need = np.arange(pend.size)
        while need.size:
            xn, _ = std_normal(rng, idx[pend[need]], T, margin)
            x[need] = xn.astype(f)
            v[need] = f(1) + cc * x[need]
            need = need[v[need] <= 0]
        v = v * v * v
        u = rng.u01_open(idx[pend]).astype(f)
        x2 = x * x
        acc = u < f(1) - f(0.0331) * x2 * x2
        slow = ~acc
        acc[slow] = np.log(u[slow]) < f(0.5) * x2[slow] + d * (
            f(1) - v[slow] + np.log(v[slow]))
        out[pend[acc]] = (boost[pend[acc]] * d * v[acc]).astype(np.float64)
        pend = pend[~acc]
    return out


Streams = namedtuple("Streams", "samples tail_mask min_margin")


def generate(dist, seed, lanes, n, tables, p0=0.0, dtype=np.float64):
    """Samples 0..n-1 of the bulk layout for `dist` in {"u64", "u01",
    "std_exponential", "std_normal", "std_gamma"} ("u64" gives the raw
    64-bit draws as uint64)."""
    live0 = min(lanes, n)
    rng = Sfc64(lane_seeds(seed, lanes)[:live0])
    out = np.empty(n, dtype=U if dist == "u64" else np.float64)
    tail = np.zeros(n, dtype=bool)
    margin = Margin()
    for base in range(0, n, lanes):
        idx = np.arange(min(lanes, n - base))
        sl = slice(base, base + idx.size)
        if dist == "u64":
            out[sl] = rng.next(idx)
        elif dist == "u01":
            out[sl] = rng.u01(idx)
        elif dist == "std_exponential":
            out[sl] = std_exponential(rng, idx, tables, margin)
        elif dist == "std_normal":
            out[sl], tail[sl] = std_normal(rng, idx, tables, margin)
        elif dist == "std_gamma":
            out[sl] = std_gamma(rng, idx, p0, tables, margin, dtype)
        else:
            raise ValueError(dist)
    return Streams(out, tail, margin.min)


def ulp_distance(a, b):
    """Distance in units in the last place between two float64 arrays
    (number of representable doubles between them), as int64."""
    def key(x):
        k = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
        return np.where(k < 0, np.int64(-(2 ** 63)) - k, k)
    return np.abs(key(a) - key(b))
