"""Host-side HIP plumbing (csrc/hip/hip_host.hpp): build the stand-alone
self-check and run it.  It needs no GPU: without a device it drives the
early-return path (every allocation fails, every destructor still runs
clean), with one it round-trips 1 KiB through DevBuf and times an empty
window."""
import os
import subprocess

from cimba_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hip_host_selfcheck(tmp_path):
    exe = str(tmp_path / "hip_host_selfcheck")
    cc = subprocess.run(
        [_build._hipcc(), "-std=c++17", "-O1", "-g",
         "-I" + os.path.join(ROOT, "cimba_amd", "csrc", "hip"),
         os.path.join(ROOT, "scripts", "hip_host_selfcheck.cpp"), "-o", exe],
        capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr[-3000:])
    assert "hip_host_selfcheck ok" in run.stdout
