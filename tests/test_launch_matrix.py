"""Every launcher instantiation reachable through the per-model entry
points computes the same trials.

The CIMBA_* knobs pick a kernel kind (wave, HBM lanes, scratch lanes,
vote-gated conv, conv with the hot state in LDS), a MINW register budget
and a grid cap.  None of them may change what a trial computes: within a
trial the event order depends on the seed alone.  Each arm is compared
with the model's first arm on every key of the result dict except the
wall-clock ones, and equality is exact.

321 trials = 256 + 64 + 1: a full 256-lane workgroup, then a full wave,
then a single live lane.  For the 64-lane LDS kernel that is five
workgroups plus one lane, for the four-wave trial-per-wavefront kernel
80 blocks plus one wave.  The grid caps (LANE_BLOCKS / CONV_BLOCKS) make
the same lanes loop over several trials.

MM1Log's kinds are pinned by tests/test_devlog.py and SpillProbe by
tests/test_gpu.py.
"""
import os
from contextlib import contextmanager

import pytest

import cimba_amd as ca

pytestmark = pytest.mark.gpu

NTRIALS = 321
WALL_CLOCK = {"elapsed_ms", "events_per_sec", "target_dwells_per_sec"}


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def run(fn, kw, arm):
    with env(**arm):
        r = fn(ntrials=NTRIALS, device=0, **kw)
    assert r["trials_ok"] == NTRIALS, (arm, r.get("first_bad_status"))
    return r


def differing_keys(ref, got):
    """Keys (wall-clock ones aside) on which two result dicts differ; a
    key present in only one of them differs."""
    keys = (set(ref) | set(got)) - WALL_CLOCK
    return sorted(k for k in keys
                  if k not in ref or k not in got or ref[k] != got[k])


def check_arms(fn, kw, arms):
    ref = run(fn, kw, arms[0])
    assert set(ref) - WALL_CLOCK, "nothing left to compare"
    for arm in arms[1:]:
        assert differing_keys(ref, run(fn, kw, arm)) == [], (arms[0], arm)
    return ref


MM1_KW = dict(num_objects=2000, seed=0x5EED1)
MM1_ARMS = [
    dict(CIMBA_MM1_LANE=0),
    dict(CIMBA_MM1_LANE=0, CIMBA_MM1_MINW=4),
    dict(CIMBA_MM1_LANE=0, CIMBA_MM1_MINW=5),
    dict(CIMBA_MM1_LANE=0, CIMBA_MM1_MINW=6),
    dict(CIMBA_MM1_LANE=1),
    dict(CIMBA_MM1_LANE=1, CIMBA_MM1_LANE_BLOCKS=1),
    dict(CIMBA_MM1_LANE=2),
    dict(CIMBA_MM1_LANE=2, CIMBA_SCRATCH_MINW=4),
    dict(CIMBA_MM1_LANE=2, CIMBA_SCRATCH_MINW=4, CIMBA_MM1_LANE_BLOCKS=1),
    dict(CIMBA_MM1_LANE=3),
    dict(CIMBA_MM1_LANE=3, CIMBA_CONV_MINW=1),
    dict(CIMBA_MM1_LANE=3, CIMBA_CONV_MINW=1, CIMBA_CONV_BLOCKS=1),
    dict(CIMBA_MM1_LANE=4),
    dict(CIMBA_MM1_LANE=4, CIMBA_LDS_MINW=2),
    dict(CIMBA_MM1_LANE=4, CIMBA_LDS_MINW=2, CIMBA_CONV_BLOCKS=2),
]

MG1_KW = dict(num_objects=2000, arr_rate=0.8, srv_mean=1.0, srv_scv=0.25,
              dist=3, seed=0x5EED2)
MG1_ARMS = [
    dict(CIMBA_MG1_LANE=0),
    dict(CIMBA_MG1_LANE=0, CIMBA_MG1_MINW=3),
    dict(CIMBA_MG1_LANE=0, CIMBA_MG1_MINW=1),
    dict(CIMBA_MG1_LANE=2),
    dict(CIMBA_MG1_LANE=2, CIMBA_SCRATCH_MINW=4),
    dict(CIMBA_MG1_LANE=3),
    dict(CIMBA_MG1_LANE=3, CIMBA_CONV_MINW=1),
    dict(CIMBA_MG1_LANE=4),
    dict(CIMBA_MG1_LANE=4, CIMBA_LDS_MINW=2),
]

JS_KW = dict(entities=1000, njobs=24, seed=0x5EED3)
JS_ARMS = [
    dict(CIMBA_JS_LANE=0),
    dict(CIMBA_JS_LANE=0, CIMBA_JS_MINW=1),
    dict(CIMBA_JS_LANE=3),
    dict(CIMBA_JS_LANE=1),
    dict(CIMBA_JS_LANE=1, CIMBA_JS_LANE_MINW=2),
    dict(CIMBA_JS_LANE=1, CIMBA_JS_LANE_MINW=3),
]


def test_mm1_arms_agree():
    check_arms(ca.mm1_gpu, MM1_KW, MM1_ARMS)


def test_mm1hot1_arms_agree_with_mm1_conv():
    """MM1Hot1 runs only on the LDS kernel; both its MINW instantiations
    must equal MM1 on the all-scratch conv kernel."""
    ref = run(ca.mm1_gpu, MM1_KW, dict(CIMBA_MM1_LANE=3))
    for arm in ({}, dict(CIMBA_LDS_MINW=2)):
        got = run(ca._C.mm1hot1_gpu, MM1_KW, arm)
        assert differing_keys(ref, got) == [], arm


def test_mg1_arms_agree():
    check_arms(ca.mg1_gpu, MG1_KW, MG1_ARMS)


def test_jobshop_arms_agree():
    check_arms(ca.jobshop_gpu, JS_KW, JS_ARMS)
