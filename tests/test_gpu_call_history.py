"""Every entry point's answer is independent of the calls before it (probes and predecessors: tests/history_cases.py, proved on
the CPU by tests/test_history_cases_host.py; the inventory of what the library keeps between calls: DESIGN.md, "State kept
between calls").

For every probe, in this order:
1. anchor -- the probe's first run in the process is held to the bar of its own test file against its reference;
2. cells -- for every predecessor the predecessor runs, then the probe again, and the probe returns the bytes of the anchor run:
   the outputs, the rows of X beyond the matrix, Y, the gramian, the failed row.  No position is excused;
3. fresh process -- one child runs every probe once and prints a digest of its bytes; the parent's anchors match it.

The comparison is bytes throughout (every probe is `exact`), so this file has no tolerance of its own.  A ValueError from a
`refused` predecessor is an answer of the API, not a fault of the device."""
import json
import os
import subprocess
import sys

import pytest

import history_cases as h

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300

_ANCHOR = {}


def anchor(gpu, name):
    """The bytes of the probe's first run in this process, kept unchanged."""
    if name not in _ANCHOR:
        out = h.PROBES[name].run(gpu)
        for a in out.values():
            a.setflags(write=False)
        _ANCHOR[name] = out
    return _ANCHOR[name]


@pytest.mark.parametrize("name", list(h.PROBES))
def test_anchor(gpu, oracle, name):
    h.PROBES[name].gate(gpu, oracle, anchor(gpu, name))


@pytest.mark.parametrize("name,predecessor", h.cells(), ids=lambda v: v.replace(":", "="))
def test_cell(gpu, oracle, name, predecessor):
    probe = h.PROBES[name]
    want = anchor(gpu, name)
    h.run_predecessor(gpu, probe, predecessor)
    got = probe.run(gpu)
    if probe.exact:
        diff = h.differing(want, got)
        assert not diff, f"{name} after {predecessor}: " + "; ".join(f"{k}: {v}" for k, v in diff.items())
    else:
        probe.gate(gpu, oracle, got)


def test_fresh_process(gpu):
    """Every probe in a process of its own that has run nothing else of its family: the bytes a history-free library gives."""
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
            "import history_cases as h; h.run_fresh()")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    lines = [line for line in out.stdout.splitlines() if line.startswith("history digests ")]
    assert out.returncode == 0 and len(lines) == 1, (out.stdout + out.stderr)[-3000:]
    fresh = json.loads(lines[0][len("history digests "):])
    assert sorted(fresh) == sorted(h.PROBES)
    differ = [name for name, p in h.PROBES.items() if p.exact and h.digest(anchor(gpu, name)) != fresh[name]]
    assert not differ, f"probes whose bytes differ from a fresh process's: {differ}"
