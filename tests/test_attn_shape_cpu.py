"""The attention's one (D, H) -> template-instance switch, checked without a GPU.

csrc/attn_shape.hpp is plain C++17: every launch function of attn_fwd.hip, attn_bwd.hip and attn_bwd_runs.hip reaches its
kernel instance through attn_for_shape<cap>.  tests/host/attn_shape.cpp walks it for both caps, every D in 1..256 and H in
{0, 1, 2, 3, 4, 8}; this module builds the program and states what each line must say.  The device-only comparison of the
code objects shows that the instances are the same kernels; this shows that each (D, H) reaches the instance it names.
"""
import os
import shutil
import subprocess

import pytest

from pfotgnrec_amd import build as _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pfotgnrec_amd", "csrc")
HEADS = (0, 1, 2, 3, 4, 8)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", _build._hipcc()) if c and shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    d = tmp_path_factory.mktemp("attn_shape")
    subprocess.check_call([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "attn_shape.cpp"), "-o", str(d / "attn_shape")])
    p = subprocess.run([str(d / "attn_shape")], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout.splitlines()


def test_caps(lines):
    """16 admits every pair (the register forms); 12 leaves out (4, 4) alone (the ring forms and the run-merged backward)."""
    assert lines[0] == "caps 16 12"


def test_every_pair_reaches_its_instance_or_none(lines):
    rows = [tuple(int(x) for x in line.split()) for line in lines[1:]]
    assert [r[:3] for r in rows] == [(cap, D, H) for cap in (16, 12) for D in range(1, 257) for H in HEADS]
    called = {16: set(), 12: set()}
    for cap, D, H, ret, calls, nr, h in rows:
        NR = -(-D // 64)
        if H in (1, 2, 4) and NR * H <= cap:
            assert (ret, calls, nr, h) == (1, 1, NR, H), (cap, D, H)
            called[cap].add((nr, h))
        else:
            assert (ret, calls, nr, h) == (0, 0, 0, 0), (cap, D, H)
    pairs = {(nr, h) for nr in (1, 2, 3, 4) for h in (1, 2, 4)}
    assert called[16] == pairs and called[12] == pairs - {(4, 4)}
