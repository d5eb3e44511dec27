"""oracle.build() under concurrent callers: the spawned ranks of tests/test_dist_cpu.py each call it, and after a fresh checkout
(the source newer than the libraries) each finds the libraries stale.  Every process must load a whole library."""
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CHILD = ("import numpy as np; from oracle import oracle; "
         "assert oracle._lib(np.float64).orc_real_bytes() == 8 and oracle._lib(np.float32).orc_real_bytes() == 4")


def test_stale_libraries_are_rebuilt_once_and_never_seen_half_written():
    from oracle import oracle
    oracle.build()
    libs = [ROOT / "oracle" / n for n in oracle._NAMES]
    old = (ROOT / "oracle" / "s360_oracle.c").stat().st_mtime - 100.0
    for f in libs:
        os.utime(f, (old, old))                                                 # stale: older than the source
    assert oracle._stale()
    procs = [subprocess.Popen([sys.executable, "-c", CHILD], cwd=str(ROOT), stderr=subprocess.PIPE, text=True) for _ in range(4)]
    errs = [(p.wait(timeout=300), p.stderr.read()[-1500:]) for p in procs]
    assert all(code == 0 for code, _ in errs), errs
    assert not oracle._stale() and not list((ROOT / "oracle").glob(".build-*"))
