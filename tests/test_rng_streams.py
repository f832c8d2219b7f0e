"""Exact per-lane stream parity for the bulk RNG kernels.

Three implementations of the same streams are pinned to each other:

  numpy reference (tests/rng_ref.py)  <->  host C++ (`_C.rng_sample_lanes`,
  the cmb::Rng code laid out as the kernel lays it out)  <->  gfx950 kernels
  (`_C.rng_sample_gpu`, `_C.rng_moments_gpu`).

Contract (profiles/r05_rng_stream_parity.md): the build uses
-ffp-contract=off, the ziggurat fast path is integer work plus one multiply,
so samples are BITWISE equal.  Only values that pass through log/pow may
differ by ulps: the normal tail beyond NOR_R (<= 4 ulp: R + x with
x = -log(u)/R carries at most 1 ulp of log error on each side plus the
roundings) and std_gamma with alpha < 1.  The sample that follows a tail
sample on the same lane is bitwise equal again, so both sides consumed the
same number of draws.  Accept/reject comparisons that involve exp/log could
in principle flip between math libraries; the CPU tests prove from the
long-double reference that for the committed seed every such comparison
has a relative margin >= 2^-40 (libraries differ by ~2^-51), which is what
allows the GPU contract to be zero mismatches.
"""
import functools
import math

import numpy as np
import pytest

import cimba_amd as ca
from tests import rng_ref

_C = ca._C
T = _C.zig_tables()

SEED = 0x5EED5EED2024
BLOCK = 256
DEEP = (2, 2 * BLOCK * 2000 + 37)       # 512 lanes, 2000+ draws per lane
WIDE = (2048, 2048 * BLOCK + 37)        # default launch, 1-2 draws per lane
TINY = [(2048, n) for n in (1, 63, 64, 65)]
MAIN_SHAPES = [DEEP, WIDE]
ALL_SHAPES = MAIN_SHAPES + TINY
ZIG_DISTS = ["u01", "std_exponential", "std_normal"]

MIN_MARGIN = 2.0 ** -40
NORMAL_TAIL_ULP = 4
# Largest ulp distance, over MAIN_SHAPES at SEED, between the host double
# std_gamma(0.5) and the same formula evaluated in long double (measured by
# test_gamma_half_reference_spread, which keeps this constant honest).  The
# device tolerance is 4x this: the reference's own spread, not a device
# measurement.
GAMMA_HALF_REF_SPREAD_ULP = 39


def shape_id(s):
    return f"b{s[0]}-n{s[1]}"


def lanes_of(shape):
    return shape[0] * BLOCK


@functools.lru_cache(maxsize=None)
def ref(dist, shape, p0=0.0, longdouble=False):
    r = rng_ref.generate(dist, SEED, lanes_of(shape), shape[1], T, p0,
                         np.longdouble if longdouble else np.float64)
    for a in (r.samples, r.tail_mask):
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def host(dist, shape, p0=0.0):
    a = _C.rng_sample_lanes(dist, p0, shape[1], SEED, lanes_of(shape))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def dev(dist, shape, p0=0.0):
    a = _C.rng_sample_gpu(dist, p0, shape[1], SEED, 0, blocks=shape[0])
    a = a["samples"]
    a.setflags(write=False)
    return a


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def where_msg(i, lanes, got, want):
    return (f"first mismatch at sample {i}: lane {i % lanes}, draw "
            f"{i // lanes}: got {got[i]!r} ({bits(got)[i]:#018x}), want "
            f"{want[i]!r} ({bits(want)[i]:#018x})")


def assert_streams(got, want, lanes, loose=None, loose_ulp=0):
    """Bitwise equality outside `loose`; inside it at most `loose_ulp`, and
    the next sample of a loose sample's lane bitwise equal again."""
    assert got.shape == want.shape
    if loose is None:
        loose = np.zeros(want.shape, dtype=bool)
    bad = (bits(got) != bits(want)) & ~loose
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{int(bad.sum())} of {bad.size} differ; "
                             + where_msg(i, lanes, got, want))
    if loose.any():
        d = rng_ref.ulp_distance(got[loose], want[loose])
        if d.max() > loose_ulp:
            i = int(np.flatnonzero(loose)[int(np.argmax(d > loose_ulp))])
            raise AssertionError(f"tail sample off by {int(d.max())} ulp > "
                                 f"{loose_ulp}; " + where_msg(i, lanes, got, want))
        nxt = np.flatnonzero(loose) + lanes
        nxt = nxt[nxt < want.size]
        nxt = nxt[~loose[nxt]]
        assert (bits(got)[nxt] == bits(want)[nxt]).all()
    return int(loose.sum())


# --------------------------------------------------------------------------
# CPU: numpy reference <-> host C++
# --------------------------------------------------------------------------

def test_seed_derivation_matches_host():
    xs = [0, 1, SEED, 2 ** 63, 2 ** 64 - 1, 0x9E3779B97F4A7C15]
    assert [int(v) for v in rng_ref.fmix64(xs)] == [ca.fmix64(x) for x in xs]
    for s in xs:
        r = rng_ref.Sfc64([s])
        zero = np.array([0])
        # the 12-round warm-up inside seed() leaves counter at 13
        assert int(r.state()[3][0]) == 13
        raw = [int(r.next(zero)[0]) for _ in range(8)]
        # full 64-bit draws pin the whole (a, b, c, counter) state
        assert raw == [ca.sfc64_raw(s, k) for k in range(8)]
        top53 = ca.rng_sample("u64", [], 8, s)
        assert [float(v >> 11) for v in raw] == list(top53)
    # the bulk lane seed, through lane 0 and a far lane of the u01 stream
    lanes = 512
    seeds = rng_ref.lane_seeds(SEED, lanes)
    g = 389
    want = ca.fmix64(SEED ^ ((g * 0x9E3779B97F4A7C15 + 1) % 2 ** 64))
    assert int(seeds[g]) == want
    u = _C.rng_sample_lanes("u01", 0.0, lanes, SEED, lanes)
    assert u[g] == ca.rng_sample("u64", [], 1, want)[0] * 2.0 ** -53


@pytest.mark.parametrize("shape", MAIN_SHAPES, ids=shape_id)
@pytest.mark.parametrize("dist", ZIG_DISTS)
def test_reference_matches_host_lanes(dist, shape):
    r = ref(dist, shape)
    ntail = assert_streams(host(dist, shape), r.samples, lanes_of(shape),
                           r.tail_mask, NORMAL_TAIL_ULP)
    if dist == "std_normal":
        # the tail mask and the value test used on the GPU side agree
        assert (r.tail_mask == (np.abs(r.samples) > T["NOR_R"])).all()
        assert ntail > 0


@pytest.mark.parametrize("shape", MAIN_SHAPES, ids=shape_id)
@pytest.mark.parametrize("dist", ["std_exponential", "std_normal"])
def test_decision_margins(dist, shape):
    # TINY shapes are prefixes of WIDE (same seed, same lanes), so these
    # two shapes cover every seed/shape the GPU tests use.  The gamma
    # streams draw their normals through the same code; their margins are
    # checked in test_gamma_half_reference_spread.
    m = ref(dist, shape).min_margin
    print(f"{dist} {shape_id(shape)}: min decision margin {m:.3e} "
          f"(2^{math.log2(m):.1f})")
    assert m >= MIN_MARGIN


def test_tail_coverage():
    r = ref("std_normal", DEEP)
    ntail = int(r.tail_mask.sum())
    nfollow = int((np.flatnonzero(r.tail_mask) + lanes_of(DEEP)
                   < r.samples.size).sum())
    nexp = int((ref("std_exponential", DEEP).samples > T["EXP_R"]).sum())
    print(f"normal tail samples {ntail} (followed on the lane: {nfollow}), "
          f"exponential samples beyond EXP_R {nexp}")
    assert ntail >= 50          # ~260 expected of 1 024 037
    assert nfollow >= 50
    assert (r.tail_mask & (r.samples > 0)).any()
    assert (r.tail_mask & (r.samples < 0)).any()
    assert nexp >= 50           # ~460 expected
    assert int(ref("std_normal", WIDE).tail_mask.sum()) >= 10


@pytest.mark.parametrize("shape", MAIN_SHAPES, ids=shape_id)
def test_gamma_reference_matches_host(shape):
    # alpha >= 1: no pow; values move only where a normal-tail deviate went
    # in, so the double-precision reference equals the host almost everywhere
    h = host("std_gamma", shape, 2.5)
    r = ref("std_gamma", shape, 2.5)
    d = rng_ref.ulp_distance(h, r.samples)
    assert d.max() <= 8
    assert (d != 0).mean() <= 0.01
    assert r.min_margin >= MIN_MARGIN


def normal_tail_share(shape):
    return float((np.abs(host("std_normal", shape)) > T["NOR_R"]).mean())


@pytest.mark.parametrize("shape", MAIN_SHAPES, ids=shape_id)
def test_gamma_cap_condition(shape):
    # the GPU test allows 1 % of gamma(2.5) samples to differ in bits; only
    # normal-tail deviates can move a value, and their share is far below
    share = normal_tail_share(shape)
    print(f"normal tail share {shape_id(shape)}: {share:.3e}")
    assert 0 < share < 1e-3


def test_gamma_half_reference_spread():
    worst = 0
    for shape in MAIN_SHAPES:
        lo = ref("std_gamma", shape, 0.5, True)
        assert lo.min_margin >= MIN_MARGIN
        d = int(rng_ref.ulp_distance(host("std_gamma", shape, 0.5),
                                     lo.samples).max())
        print(f"gamma(0.5) {shape_id(shape)}: host double vs long double "
              f"formula: max {d} ulp")
        worst = max(worst, d)
    assert 1 <= worst <= GAMMA_HALF_REF_SPREAD_ULP


def test_blocks_argument_validated():
    for bad in (0, -1, 2049):
        with pytest.raises(ValueError):
            _C.rng_sample_gpu("u01", 0.0, 8, 1, 0, blocks=bad)
        with pytest.raises(ValueError):
            _C.rng_moments_gpu("u01", 0.0, 8, 1, 0, 0, blocks=bad)


# --------------------------------------------------------------------------
# GPU: kernels <-> host C++
# --------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=shape_id)
@pytest.mark.parametrize("dist", ZIG_DISTS)
def test_gpu_streams_match_host(dist, shape):
    h = host(dist, shape)
    g = dev(dist, shape)
    # tail samples are identified by the host value
    loose = np.abs(h) > T["NOR_R"] if dist == "std_normal" else None
    if loose is not None and loose.any():
        print(f"{dist} {shape_id(shape)}: {int(loose.sum())} tail "
              f"samples, max device-host distance "
              f"{int(rng_ref.ulp_distance(g[loose], h[loose]).max())} ulp")
    assert_streams(g, h, lanes_of(shape), loose, NORMAL_TAIL_ULP)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MAIN_SHAPES, ids=shape_id)
def test_gpu_gamma_matches_host(shape):
    h = host("std_gamma", shape, 2.5)
    g = dev("std_gamma", shape, 2.5)
    d = rng_ref.ulp_distance(g, h)
    print(f"gamma(2.5) {shape_id(shape)}: max {int(d.max())} ulp, "
          f"{int((d != 0).sum())} of {d.size} not bitwise equal")
    if d.max() > 8:
        i = int(np.argmax(d > 8))
        raise AssertionError(where_msg(i, lanes_of(shape), g, h))
    assert (d != 0).mean() <= 0.01


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MAIN_SHAPES, ids=shape_id)
@pytest.mark.parametrize("mean", [4.0, 12.0])
def test_gpu_poisson_matches_host(mean, shape):
    # Knuth (mean < 10) and PTRS branches; integers, so exact
    assert_streams(dev("poisson", shape, mean), host("poisson", shape, mean),
                   lanes_of(shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MAIN_SHAPES, ids=shape_id)
def test_gpu_gamma_half_matches_host(shape):
    h = host("std_gamma", shape, 0.5)
    g = dev("std_gamma", shape, 0.5)
    d = rng_ref.ulp_distance(g, h)
    tol = 4 * GAMMA_HALF_REF_SPREAD_ULP
    print(f"gamma(0.5) {shape_id(shape)}: max device-host distance "
          f"{int(d.max())} ulp (tolerance {tol})")
    if d.max() > tol:
        i = int(np.argmax(d > tol))
        raise AssertionError(where_msg(i, lanes_of(shape), g, h))


@functools.lru_cache(maxsize=None)
def power_sums(dist, shape):
    """Exact (fsum) power sums of the materialised device samples; the
    powers themselves are double products (<= 2 roundings per term, part of
    the +16 allowance below)."""
    x = dev(dist, shape)
    x2 = x * x
    pw = [x, x2, x2 * x, x2 * x2]
    return ([math.fsum(p) for p in pw], [math.fsum(np.abs(p)) for p in pw],
            float(x.min()), float(x.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=shape_id)
@pytest.mark.parametrize("dist", ["std_normal", "std_exponential"])
@pytest.mark.parametrize("mfma", [0, 1])
def test_gpu_moments_exact(mfma, dist, shape):
    blocks, n = shape
    lanes = lanes_of(shape)
    sums, abs_sums, mn, mx = power_sums(dist, shape)
    r = _C.rng_moments_gpu(dist, 0.0, n, SEED, 0, mfma, blocks=blocks)
    assert r["n"] == float(n)
    assert r["min"] == mn and r["max"] == mx
    # each lane's sequential sum + wave butterfly + per-wave atomics + the
    # MFMA's inner K sum, every addition at most half an ulp of the running
    # magnitude
    terms = -(-n // lanes) + lanes // 64 + 16
    for k, name in enumerate(("s1", "s2", "s3", "s4")):
        tol = terms * 2.0 ** -53 * abs_sums[k]
        err = abs(r[name] - sums[k])
        print(f"mfma={mfma} {dist} {shape_id(shape)} {name}: err {err:.3e} "
              f"tol {tol:.3e}")
        assert err <= tol, (name, r[name], sums[k], err, tol)
    assert r["mean"] == r["s1"] / r["n"]
