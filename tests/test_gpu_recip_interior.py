"""The area reciprocal of an interior pose's fragment test (pcore_fdiv.h, recip_interior: the compiler's division
sequence for 1.0f / Y without its scaling steps, the raw v_rcp_f32 where Y = 0) equals `1.0f / Y` bit for bit on the
GPU: tools/recip_check.hip walks every float Y with |Y| in [2^-50, 2^29) -- the bound of an interior pose, 79
exponents x 2^23 mantissas -- in both signs, and +-0, in one launch.  The binary is built by
__graft_entry__.build()."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_recip_interior_matches_ieee_division_exhaustively():
    exe = os.path.join(ROOT, "tools", "bin", "recip_check")
    if not os.path.exists(exe):
        pytest.fail("tools/bin/recip_check missing: run __graft_entry__.build()")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(r.stdout)
    assert res["values"] == 79 * 2 * 2 ** 23 + 2
    assert r.returncode == 0 and res["mismatches"] == 0 and res["zero_mismatches"] == 0, r.stdout + r.stderr
