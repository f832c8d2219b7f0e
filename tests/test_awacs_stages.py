"""AWACS radar pipeline, per target and per stage: the unmodified device
functions (beamform_tile, beamform_tile_idx, dwell_physics_wave,
dwell_physics_block and the whole-run kernels) against the host engine and
an fp64 reference, target by target.

Plain f32 arithmetic is shared by host and device (-ffp-contract=off), so
positions, altitudes and LOS verdicts are compared BITWISE; only
atan2f/sinf/cosf/expf differ (OCML vs libm), and the tolerances for what
depends on them are measured on the CPU (tests/awacs_cases.py; figures in
profiles/r06_awacs_stage_parity.md).  The unmarked tests here are those
measurements and the host-only conditions the GPU tests rely on.
"""
import numpy as np
import pytest

import cimba_amd as ca
from tests import awacs_cases as ac

C = ca._C
ids = lambda cases: [c["name"] for c in cases]


# ---------------------------------------------------------------- CPU side
def test_tol_bf_is_four_times_host_error():
    worst = 0.0
    for n in ac.BF_COUNTS:
        r = C.awacs_power_check(ntargets=n, seed=ac.BF_SEED, gpu=False)
        assert r["nt"] == min(n, ac.MAX_T)
        bf64 = r["bf_f64"]
        assert 100.0 < bf64.min() and bf64.max() <= 256.0  # well conditioned
        worst = max(worst, ac.rel_err(r["host_bf_f32"], bf64).max())
        # the composed power adds three f32 roundings to the same error
        assert (ac.rel_err(r["host_f32"], r["host_f64"]) <= ac.TOL_BF).all()
    print("host f32 vs fp64 raw bf: worst rel err %.6e" % worst)
    assert worst == pytest.approx(ac.BF_HOST_REL_ERR, rel=0.02)
    assert ac.TOL_BF == 4.0 * ac.BF_HOST_REL_ERR


@pytest.fixture(scope="module")
def host_runs():
    return {c["name"]: ac.run_dwell(c, "host") for c in ac.DWELL_CASES}


@pytest.fixture(scope="module")
def host_free_runs():
    return {c["name"]: ac.run_dwell(c, "host_free") for c in ac.FREE_CASES}


def test_host_intermediates_reproduce_physics_all(host_runs, host_free_runs):
    for r in host_runs.values():
        ac.check_host_consistency(r, pipeline=True)
    for r in host_free_runs.values():
        ac.check_host_consistency(r, pipeline=False)


def test_cases_reach_the_edges(host_runs):
    illum = {k: int((r["stage"] > 0).sum()) for k, r in host_runs.items()}
    clear = {k: int((r["stage"] == 3).sum()) for k, r in host_runs.items()}
    # gate: a few of 1000 pass; two cases with an empty survivor list
    assert illum["small_t0"] == 0 and illum["small_t4"] == 0
    assert all(0 < illum["default_t%g" % t] < 30
               for t in (0.0, 1.0, 2.52, 7.3, 9.96))
    assert clear["default_t2.52"] == 0 < illum["default_t2.52"]
    # wide beam: everyone illuminated, the survivor list full at 1024
    for nt in (1, 63, 64, 65, 255, 256, 257, 1000, 1024):
        assert illum["wide_nt%d" % nt] == nt
    assert clear["wide_nt1000"] > 200
    # dt = 20 s: several percent wrap at +-area
    r = host_runs["wide_dt20"]
    nt = r["nt"]
    moved = np.maximum(np.abs(r["host"]["x"][:nt] - r["init"]["x"][:nt]),
                       np.abs(r["host"]["y"][:nt] - r["init"]["y"][:nt]))
    assert 0.03 * nt < (moved > 5.0e4).sum() < 0.15 * nt
    # eight dwell indices redraw the same clear set at different u
    us = [host_runs["wide_dwl%d" % d]["u"] for d in range(8)]
    assert all(not np.array_equal(us[0], u) for u in us[1:])


def test_host_has_no_target_in_the_gate_band(host_runs):
    """Seeds are chosen so that the host alone excuses nobody: the
    expected count is ~1e-3 per case (2 edges x 3.8e-6 rad x nt / 2 pi)."""
    for name, r in host_runs.items():
        n = int((np.abs(r["gate_margin"]) <= ac.GATE_BAND).sum())
        assert n == 0, (name, n)


def test_host_detections_within_pd_band_cap(host_runs, host_free_runs):
    """The host f32 decisions against the fp64 pd: every disagreement lies
    inside BAND_PD by construction; the cap the device must meet (1 % of
    the clear targets) holds for the host alone."""
    for name, r in list(host_runs.items()) + list(host_free_runs.items()):
        clear = np.asarray(r["stage"]) == 3
        band = ac.pd_band(r, clear)
        d32 = (r["u"] < r["pd"]) & clear
        d64 = (r["u"] < r["pd_f64"]) & clear
        differ = d32 != d64
        print("%s: clear %d BAND_PD %.3e host-vs-fp64 differing %d" %
              (name, int(clear.sum()), band, int(differ.sum())))
        assert (np.abs(r["u"] - r["pd"])[differ] <= band).all()
        assert differ.sum() <= ac.DET_EXCUSED_FRAC * clear.sum(), name
        assert 0.0 <= band <= 4.0  # pd lies in [0, 1]


def test_sum_tolerances_are_four_times_host_error(host_runs):
    wp = wc = 0.0
    for name, r in host_runs.items():
        h = r["host"]
        if r["sum_power_f64"] > 0.0:
            wp = max(wp, abs(h["sum_power"] - r["sum_power_f64"]) /
                     r["sum_power_f64"])
            wc = max(wc, abs(h["sum_clutter"] - r["sum_clutter_f64"]) /
                     r["sum_clutter_f64"])
    print("host f32 vs fp64 sums: power %.6e clutter %.6e" % (wp, wc))
    assert wp == pytest.approx(ac.SUM_POWER_HOST_REL_ERR, rel=0.02)
    assert wc == pytest.approx(ac.SUM_CLUTTER_HOST_REL_ERR, rel=0.02)


STATE_KW = dict(ntrials=4, duration=5.0, ntargets=512, seed=11)


@pytest.fixture(scope="module")
def host_state():
    return {k: C.awacs_host_state(kernel=k, **STATE_KW)
            for k in ("block", "free")}


def test_host_state_dump_deterministic(host_state):
    a = host_state["block"]
    b = C.awacs_host_state(kernel="wave", **STATE_KW)  # same host pipeline
    for k in ("x", "y", "vx", "vy", "det_cnt", "detections"):
        assert a[k].tobytes() == b[k].tobytes(), k
    # the dump is the run awacs_host aggregates
    for kernel, terrain in (("block", 1), ("free", 0)):
        s = host_state[kernel]
        h = C.awacs_host(threads=2, terrain=terrain, **STATE_KW)
        for k in ("total_detections", "total_dwells", "total_maneuvers",
                  "total_events", "total_illuminated", "total_shielded",
                  "sum_power", "sum_clutter", "trials_ok"):
            assert s[k] == h[k], (kernel, k)
        assert s["x"].shape == (4, 512)
        assert np.array_equal(s["det_cnt"].sum(axis=1), s["detections"])
        assert np.abs(s["x"]).max() <= 5.0e4 and np.abs(s["y"]).max() <= 5.0e4


def test_state_bindings_reject_bad_arguments():
    with pytest.raises(ValueError):
        C.awacs_host_state(kernel="lane", **STATE_KW)
    with pytest.raises(ValueError):
        C.awacs_host_state(ntrials=4096, kernel="block")
    with pytest.raises(ValueError):
        C.awacs_dwell_check(ntargets=8, seed=1, now=0.0, dt=0.04, dwl=0,
                            mode="scalar")


# ---------------------------------------------------------------- GPU side
@pytest.mark.gpu
@pytest.mark.parametrize("nt", ac.BF_COUNTS)
def test_beamform_tile_per_target(nt):
    r = C.awacs_power_check(ntargets=nt, seed=ac.BF_SEED, device=0)
    n = r["nt"]
    assert n == min(nt, ac.MAX_T)  # 1025 clamps to MAX_T
    for sfx in ("", "_devinit"):
        assert r["device_nt" + sfx] == n
        bf = r["device_bf" + sfx]
        e_bf = ac.rel_err(bf[:n], r["bf_f64"])
        e_pw = ac.rel_err(r["device_mfma" + sfx], r["host_f64"])
        print("nt %d%s: worst rel err bf %.3e composed %.3e" %
              (nt, sfx, e_bf.max(), e_pw.max()))
        assert (e_bf <= ac.TOL_BF).all(), np.flatnonzero(e_bf > ac.TOL_BF)[:8]
        assert (e_pw <= ac.TOL_BF).all(), np.flatnonzero(e_pw > ac.TOL_BF)[:8]
        full = r["device_pow_full" + sfx]
        assert full.shape == (ac.MAX_T,)
        assert not ac.bits(full)[n:].any()  # exactly +0 past nt
    # host-initialised state: bf past nt keeps the sentinel bit pattern
    assert (ac.bits(r["device_bf"])[n:] == ac.bits(np.float32([-1.0]))[0]).all()


IDX_COUNTS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130, 1024]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["tiled", "one_by_one"])
@pytest.mark.parametrize("cnt", IDX_COUNTS)
def test_beamform_tile_idx_lists(cnt, mode):
    # a random permutation with gaps (none left at cnt = MAX_T)
    rng = np.random.default_rng(1000 + cnt)
    idx = rng.permutation(ac.MAX_T)[:cnt].astype(np.int32)
    r = C.awacs_bfidx_check(ntargets=ac.MAX_T, seed=ac.BF_SEED,
                            idx=idx.tolist(), mode=mode, device=0)
    bf = r["device_bf"]
    listed = np.zeros(ac.MAX_T, dtype=bool)
    listed[idx] = True
    sent = ac.bits(np.float32([-1.0]))[0]
    assert (ac.bits(bf)[~listed] == sent).all(), \
        np.flatnonzero(ac.bits(bf)[~listed] != sent)[:8]
    err = ac.rel_err(bf[listed], r["bf_f64"][listed])
    print("cnt %d mode %d: worst rel err %.3e" %
          (cnt, mode, err.max() if cnt else 0.0))
    assert (err <= ac.TOL_BF).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ac.PIPELINE_MODES)
@pytest.mark.parametrize("case", ac.DWELL_CASES, ids=ids(ac.DWELL_CASES))
def test_one_dwell_pipeline(case, mode):
    r = ac.run_dwell(case, mode)
    ac.check_pipeline(r, "%s/%s" % (case["name"], mode))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ac.FREE_CASES, ids=ids(ac.FREE_CASES))
def test_one_dwell_free_space(case):
    r = ac.run_dwell(case, "free")
    ac.check_free(r, case["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["block", "wave", "free"])
def test_whole_run_end_state(kernel, host_state):
    """4 trials x 125 dwells x 512 targets: lane 0 writes the maneuver
    velocities and the clock, the physics lanes read them after the
    vmcnt(0) wait and the agent-scope acquire.  One stale vx or dt on one
    target in one dwell leaves x or y off by at least an ulp."""
    g = C.awacs_gpu_state(kernel=kernel, device=0, **STATE_KW)
    h = host_state["free" if kernel == "free" else "block"]
    assert g["trials_ok"] == 4
    for k in ("total_dwells", "total_maneuvers", "total_events"):
        assert g[k] == h[k], k
    for k in ("vx", "vy", "x", "y"):
        bad = np.argwhere(g[k].view(np.uint32) != h[k].view(np.uint32))
        assert bad.size == 0, (k, len(bad), bad[:8])
    assert np.array_equal(g["det_cnt"].sum(axis=1), g["detections"])
    dist = int(np.abs(g["det_cnt"].astype(np.int64) -
                      h["det_cnt"].astype(np.int64)).sum())
    print("%s: detections dev %d host %d per-target L1 distance %d" %
          (kernel, g["total_detections"], h["total_detections"], dist))
    assert dist <= 0.03 * h["total_detections"]
