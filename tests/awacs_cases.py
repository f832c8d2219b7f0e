"""Shared cases, tolerances and checks of the AWACS per-target / per-stage
parity tests (tests/test_awacs.py, tests/test_awacs_stages.py).

Every tolerance here is 4 x an error of the HOST f32 path against the fp64
reference, measured on the CPU over exactly the cases below; the unmarked
tests in test_awacs_stages.py re-measure them and fail if a constant no
longer matches (profiles/r06_awacs_stage_parity.md has the figures).  None
comes from what the device returns.
"""
import math

import numpy as np

import cimba_amd as ca

MAX_T = 1024
BF_SEED = 42
BF_COUNTS = [1, 15, 16, 17, 63, 64, 65, 100, 1000, 1024, 1025]

# largest per-target |target_bf_f32 - bf_f64| / bf_f64 over BF_COUNTS at
# BF_SEED (host f32 vs fp64; both f32 paths share the rounded phase
# pi * e * s that dominates it), and 4 x that for the MFMA accumulation
# order and OCML-vs-libm ulps
BF_HOST_REL_ERR = 3.7977962018687826e-06
TOL_BF = 4.0 * BF_HOST_REL_ERR

# beam gate: atan2f is the only operation host and device do not share; a
# target may change sides only within 16 f32 ulps of pi of the gate edge
GATE_BAND = 16 * float(np.spacing(np.float32(math.pi)))  # 3.8e-6 rad
GATE_MAX_EXCUSED = 2

# sum_power / sum_clutter of one dwell: largest relative error of the host
# f32 sums against the fp64 sums over DWELL_CASES (one bound for all cases:
# a single case's own error can be below one f32 ulp by cancellation)
SUM_POWER_HOST_REL_ERR = 1.0645798738292907e-06
SUM_CLUTTER_HOST_REL_ERR = 1.413745802266357e-06
TOL_SUM_POWER = 4.0 * SUM_POWER_HOST_REL_ERR
TOL_SUM_CLUTTER = 4.0 * SUM_CLUTTER_HOST_REL_ERR

DET_EXCUSED_FRAC = 0.01  # of the case's clear targets

TWO_PI = 2.0 * math.pi
DWELL = 0.04


def _case(name, nt, seed, now, dt=DWELL, dwl=None, beamwidth=None):
    return dict(name=name, ntargets=nt, seed=seed, now=now, dt=dt,
                dwl=int(round(now / DWELL)) if dwl is None else dwl,
                beamwidth=beamwidth)


# One dwell each.  Default beam: ~0.8 % of the targets pass the gate; the
# two "small" cases at now = 0 and 4 illuminate nobody (empty survivor
# list).  Wide beam (2 pi): every target is illuminated, a quarter is
# LOS-clear; nt = 1024 fills the survivor list exactly and the block
# kernel's chunking sees empty (nt <= 64 with 2 or 4 waves) and partial
# chunks.  dt = 20 s wraps ~6 % of the targets at +-area.  dwl 0..7 redraw
# the same 271 clear targets' pd at eight different u.
DWELL_CASES = (
    [_case("default_t%g" % now, 1000, 5, now)
     for now in (0.0, 1.0, 2.52, 7.3, 9.96)] +
    [_case("small_t%g" % now, 64, 5, now) for now in (0.0, 1.0, 4.0)] +
    [_case("wide_nt%d" % nt, nt, 7, 1.0, beamwidth=TWO_PI)
     for nt in (1, 63, 64, 65, 255, 256, 257, 1000, 1024)] +
    [_case("wide_dt20", 1000, 9, 20.0, dt=20.0, dwl=1, beamwidth=TWO_PI)] +
    [_case("wide_dwl%d" % d, 1000, 7, 1.0, dwl=d, beamwidth=TWO_PI)
     for d in range(8)]
)
FREE_CASES = [
    _case("free_nt%d" % nt, nt, 7, 1.0, dwl=2)
    for nt in (1, 63, 64, 65, 1000, 1024)
] + [_case("free_dt20", 1000, 9, 20.0, dt=20.0, dwl=1)]

PIPELINE_MODES = ("wave", "block1", "block2", "block4")


def run_dwell(case, mode, device=0):
    kw = {k: v for k, v in case.items() if k != "name"}
    return ca._C.awacs_dwell_check(mode=mode, device=device, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rel_err(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref) / ref


def pd_band(r, sel):
    """BAND_PD of a case: 4 x the largest |pd_f32 - pd_f64| over `sel`."""
    if not sel.any():
        return 0.0
    return 4.0 * float(np.abs(r["pd"][sel] - r["pd_f64"][sel]).max())


def host_sets(r):
    nt = r["nt"]
    stage = np.asarray(r["stage"])
    return nt, stage > 0, stage == 3


def check_host_consistency(r, pipeline):
    """The per-target intermediates the binding computes with the model's
    static functions must reproduce what AWACS::physics_all did."""
    nt, illum, clear = host_sets(r)
    h, init = r["host"], r["init"]
    alt_s, bf_s = bits(init["alt"])[0], bits(init["bf"])[0]
    det = (r["u"] < r["pd"]) & clear
    assert np.array_equal(h["det_cnt"][:nt], det.astype(np.uint32))
    assert h["detections"] == int(det.sum())
    assert h["dwells"] == init["dwells"] + 1
    assert (bits(h["bf"]) == bf_s).all()  # the host path never stores bf
    if pipeline:
        assert np.array_equal(bits(h["alt"])[:nt] != alt_s, illum)
        assert h["illuminated"] == int(illum.sum())
        assert h["shielded"] == int((np.asarray(r["stage"]) == 2).sum())
    else:
        assert clear.all() and h["illuminated"] == 0 and h["shielded"] == 0
        assert (bits(h["alt"]) == alt_s).all()


def check_common(r):
    """Kinematics and the fields a dwell must not touch (every mode)."""
    nt = r["nt"]
    dev, host, init = r["dev"], r["host"], r["init"]
    assert dev["nt"] == nt == host["nt"]
    # kinematics: plain f32 arithmetic shared by host and device
    for k in ("x", "y"):
        bad = np.flatnonzero(bits(dev[k]) != bits(host[k]))
        assert bad.size == 0, (k, bad[:8], dev[k][bad[:8]], host[k][bad[:8]])
    for k in ("vx", "vy", "rcs", "wr", "wi"):
        assert np.array_equal(bits(dev[k]), bits(init[k])), k
    assert dev["dwells"] == init["dwells"] + 1 == host["dwells"]
    assert dev["last_t"] == host["last_t"]
    assert dev["maneuvers"] == init["maneuvers"]


def check_detections(r, dev_clear, host_clear, label):
    nt = r["nt"]
    dev, host, init = r["dev"], r["host"], r["init"]
    dc = np.asarray(dev["det_cnt"])
    assert (dc <= 1).all() and not dc[nt:].any()
    assert not dc[:nt][~dev_clear].any()  # only clear targets are drawn
    assert int(dc.sum()) == dev["detections"] - init["detections"]
    both = dev_clear & host_clear
    differ = (dc[:nt] != np.asarray(host["det_cnt"])[:nt]) & both
    band = pd_band(r, host_clear)
    near = np.abs(r["u"] - r["pd"]) <= band
    bad = np.flatnonzero(differ & ~near)
    print("%s: clear %d det dev %d host %d differing %d BAND_PD %.3e" %
          (label, int(both.sum()), int(dc.sum()), host["detections"],
           int(differ.sum()), band))
    assert bad.size == 0, (bad[:8], r["u"][bad[:8]], r["pd"][bad[:8]])
    assert differ.sum() <= DET_EXCUSED_FRAC * host_clear.sum()


def check_pipeline(r, label=""):
    """One pipeline dwell (wave / block modes) against the host."""
    check_common(r)
    nt, host_illum, host_clear = host_sets(r)
    dev, host, init = r["dev"], r["host"], r["init"]
    alt_s, bf_s = bits(init["alt"])[0], bits(init["bf"])[0]
    dalt, dbf = bits(dev["alt"]), bits(dev["bf"])
    assert (dalt[nt:] == alt_s).all() and (dbf[nt:] == bf_s).all()
    dev_illum = dalt[:nt] != alt_s
    dev_clear = dbf[:nt] != bf_s

    # beam gate
    diff = dev_illum != host_illum
    in_band = np.abs(r["gate_margin"]) <= GATE_BAND
    bad = np.flatnonzero(diff & ~in_band)
    assert bad.size == 0, (bad[:8], r["gate_margin"][bad[:8]])
    assert diff.sum() <= GATE_MAX_EXCUSED
    assert dev["illuminated"] - init["illuminated"] == int(dev_illum.sum())

    # horizon and LOS
    common = dev_illum & host_illum
    assert np.array_equal(dalt[:nt][common], bits(host["alt"])[:nt][common])
    assert not dev_clear[~dev_illum].any()
    assert np.array_equal(dev_clear[common], host_clear[common])
    same_sets = not diff.any()
    if same_sets:
        assert dev["illuminated"] == host["illuminated"]
        assert dev["shielded"] == host["shielded"]
    both = dev_clear & host_clear
    err = rel_err(dev["bf"][:nt][both], r["bf_f64"][both])
    print("%s: illum %d clear %d gate-excused %d worst bf err %.3e" %
          (label, int(dev_illum.sum()), int(dev_clear.sum()),
           int(diff.sum()), err.max() if err.size else 0.0))
    assert (err <= TOL_BF).all()

    check_detections(r, dev_clear, host_clear, label)

    # diagnostics (the survivor sets are identical here)
    if same_sets:
        for key, tol in (("sum_clutter", TOL_SUM_CLUTTER),
                         ("sum_power", TOL_SUM_POWER)):
            d, h = dev[key], host[key]
            print("%s: %s dev %.9e host %.9e rel %.3e" %
                  (label, key, d, h, abs(d - h) / h if h else 0.0))
            assert abs(d - h) <= tol * h, key


def check_free(r, label=""):
    """One free-space dwell: all-target beamform_tile on the rows the
    kinematics loop has just written."""
    check_common(r)
    nt = r["nt"]
    dev, host, init = r["dev"], r["host"], r["init"]
    bf_s = bits(init["bf"])[0]
    assert np.array_equal(bits(dev["alt"]), bits(init["alt"]))
    assert (bits(dev["bf"])[nt:] == bf_s).all()
    for k in ("illuminated", "shielded", "sum_clutter"):
        assert dev[k] == init[k], k
    # fp64 from the post-kinematics positions
    err = rel_err(dev["bf"][:nt], r["bf_f64"])
    r2 = (dev["x"][:nt] * dev["x"][:nt] + dev["y"][:nt] * dev["y"][:nt] +
          np.float32(1.0))
    composed = dev["bf"][:nt] * dev["rcs"][:nt] / (r2 * r2)  # the f32 steps
    assert composed.dtype == np.float32
    perr = rel_err(composed, r["pow_f64"])
    print("%s: worst bf err %.3e composed %.3e" %
          (label, err.max(), perr.max()))
    assert (err <= TOL_BF).all() and (perr <= TOL_BF).all()
    ref = r["sum_power_f64"]
    assert abs(dev["sum_power"] - ref) <= TOL_BF * ref
    allc = np.ones(nt, dtype=bool)
    check_detections(r, allc, allc, label)
