"""The step's issue order, checked without a GPU.

csrc/tgn.hip holds no kernel: compiled host-only it is a plain object, and tests/host/step_trace.cpp links it against recorders
of everything it calls.  The program runs a fixed list of scenarios and writes, per scenario, one line per launch, memset,
event record and event wait that tgn.hip queued.  This module builds it and asserts what tgn.hip's own comments claim of that
order.  ``PFO_STEP_TRACE_TGN`` names another tgn.hip (a parent commit's, say) to hold to the same properties; two versions
queue the same step iff ``diff -r`` of their log directories is empty.
"""
import os
import re
import shutil
import subprocess

import pytest

from pfotgnrec_amd import build as _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pfotgnrec_amd", "csrc")
TGN = os.environ.get("PFO_STEP_TRACE_TGN") or os.path.join(CSRC, "tgn.hip")

# events one call records (or binds to a launch) and waits for itself; pc_a / pc_b are recorded by pfo_tgn_refresh and waited for
# by later forwards, which tgn.hip documents as no-ops when no refresh is outstanding
PER_CALL = {"fork", "fold_done", "seg_done", "tn_a", "tn_b", "tn_a_done", "done2", "done", "gru_done", "comp_done", "main_done"} \
    | {"layer[%d]" % l for l in range(5)}


@pytest.fixture(scope="module")
def logs(tmp_path_factory):
    hipcc = _build._hipcc()
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("step_trace")
    flags = ["-O1", "--offload-arch=" + _build.ARCH, "-x", "hip", "--cuda-host-only", "-std=c++17", "-I", CSRC]
    for src, obj in ((TGN, "tgn.o"), (os.path.join(ROOT, "tests", "host", "step_trace.cpp"), "step_trace.o")):
        subprocess.check_call([hipcc] + flags + ["-c", src, "-o", str(d / obj)])
    # (no HIP runtime: every HIP call of the object is one of the program's recorders)
    subprocess.check_call([hipcc, "-no-hip-rt", str(d / "step_trace.o"), str(d / "tgn.o"), "-o", str(d / "step_trace")])
    runs = []
    for k in range(2):
        out = d / ("run%d" % k)
        out.mkdir()
        p = subprocess.run([str(d / "step_trace"), str(out)], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        assert all(line.split()[1] == "0" for line in p.stdout.splitlines()), p.stdout
        runs.append({f[:-4]: (out / f).read_bytes() for f in sorted(os.listdir(out))})
    return runs


def _ops(text):
    """(kind, stream, event) per queued action, in issue order.  A launcher's descriptor lines (indented) belong to the launch
    above them; an event bound to a launch (arm .. launch .. disarm) is a record behind that launch."""
    ops, armed = [], None
    for line in text.decode().splitlines():
        if line.startswith(" "):
            continue
        kind = line.split(" ", 1)[0]
        stream = re.search(r" stream=(\S+)", line)
        event = re.search(r" event=(\S+)", line)
        stream, event = stream and stream.group(1), event and event.group(1)
        if kind == "arm":
            assert armed is None, "two events armed at once"
            armed = event
        elif kind == "cancel":
            armed = None
        elif kind == "disarm":
            assert armed is not None, "disarm without an armed event"
            ops.append(("record", stream, armed))
            armed = None
        elif kind in ("scenario", "range_push", "range_pop", "mark", "hipStreamCreateWithPriority", "hipEventCreateWithFlags"):
            continue
        elif kind in ("record", "wait"):
            ops.append((kind, stream, event))
        else:
            assert stream not in (None, "null", "UNKNOWN"), line
            ops.append(("launch", stream, None))
    assert armed is None, "an armed event was left behind"
    return ops


def test_scenarios_run_and_repeat(logs):
    assert len(logs[0]) > 60 and "plain" in logs[0] and "loop" in logs[0]
    assert logs[0] == logs[1]                                    # byte for byte, scenario by scenario
    for name, text in logs[0].items():
        assert b"UNKNOWN" not in text, name                      # every pointer, stream and event is one the scenario handed in


def test_everything_is_joined(logs):
    """After the closing pfo_tgn_join every launch, memset and record of the scenario, on any stream, is ordered before the
    tail of the caller's stream: stream order + record -> wait edges, as vector clocks."""
    for name, text in logs[0].items():
        if name == "setup":
            continue
        clock, at_record, issued = {}, {}, []
        for kind, stream, event in _ops(text):
            vc = clock.setdefault(stream, {})
            if kind == "wait":
                for s, t in at_record.get(event, {}).items():
                    vc[s] = max(vc.get(s, 0), t)
                continue
            vc[stream] = vc.get(stream, 0) + 1
            issued.append((stream, vc[stream], kind, event))
            if kind == "record":
                at_record[event] = dict(vc)
        tail = clock["main"]
        left = [op for op in issued if tail.get(op[0], 0) < op[1]]
        assert not left, "%s: not ordered before the caller's stream's tail: %s" % (name, left[:5])


def test_per_call_events_are_recorded_before_they_are_awaited(logs):
    for name, text in logs[0].items():
        recorded = set()
        for kind, stream, event in _ops(text):
            if kind == "record":
                recorded.add(event)
            elif kind == "wait" and event in PER_CALL:
                assert event in recorded, "%s: %s waits for %s, which nothing in the scenario recorded" % (name, stream, event)
