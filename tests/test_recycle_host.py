"""CPU: the recycling model (tools/walk_model.cpp) on the Cornell
box with a reduced block count — every ray that a capped pass sends back on
its queue finishes with the walk's (found, t, prim), for caps 0 ... 3 in both
variants, and no level's queue passes kStreamCap — and the host's report of
the cap (mrt_debug_sweep_cap) with its diagnostic switch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_CAP = 128              # kernels.h kStreamCap
SWEEP_LEAVES = 32             # mrt_layout.h kSweepLeaves
BLOCKS = 300


@pytest.fixture(scope="module")
def model_output(mrt_mod, tmp_path_factory):
    """tools/walk_model.cpp built by its own build line and run once."""
    out = str(tmp_path_factory.mktemp("recycle_model") / "walk_model")
    csrc = os.path.join(ROOT, "metal-renderer_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + csrc,
                    os.path.join(ROOT, "tools", "walk_model.cpp"), os.path.join(csrc, "scene.cpp"),
                    os.path.join(csrc, "bvh.cpp"), "-o", out, "-lpthread"], check=True)
    r = subprocess.run([out, mrt_mod.scene_path("cornellbox"), str(BLOCKS)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_recycled_rays_finish_with_the_walks_answer_within_the_queue_bound(model_output):
    rows = {}
    for line in model_output.splitlines():
        m = re.match(r"\s+(unbounded|cap \d(?: keys)?)\s+(\d+) calls .* recycled ([\d.]+) % of rays, .* most passes (\d+); "
                     r"longest queue (\d+); mismatches (\d+) of (\d+)", line)
        if m:
            rows[m.group(1)] = [float(x) for x in m.groups()[1:]]
    assert set(rows) == {"unbounded", "cap 1", "cap 2", "cap 3", "cap 0 keys", "cap 1 keys", "cap 2 keys", "cap 3 keys"}
    rays = rows["unbounded"][5]
    assert rays >= BLOCKS * 64
    for name, (calls, recycled, passes, queue, mismatches, n) in rows.items():
        assert mismatches == 0 and n == rays, name          # the same rays under every cap, all answered as the walk does
        assert queue <= STREAM_CAP, name
        assert calls >= rows["unbounded"][0], name
    assert rows["unbounded"][1] == 0 and rows["unbounded"][2] == 1
    assert rows["cap 0 keys"][1] > rows["cap 3 keys"][1] > 0 and rows["cap 0 keys"][2] >= 3   # recycled more than once
    total = next(l for l in model_output.splitlines() if l.startswith("recycling vs walk:"))
    m = re.match(r"recycling vs walk: mismatches (\d+), longest queue (\d+) of (\d+) slots", total)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) <= int(m.group(3)) == STREAM_CAP


def test_sweep_cap_report_and_switch(mrt_mod, monkeypatch):
    monkeypatch.delenv("MRT_SWEEP_CAP", raising=False)
    s = mrt_mod.Scene("cornellbox", device=-1)
    default = mrt_mod.debug_sweep_cap(s)
    s.close()
    assert default == SWEEP_LEAVES                          # the product never recycles
    for value, want in (("0", 0), ("2", 2), ("32", SWEEP_LEAVES), ("1000", SWEEP_LEAVES)):
        monkeypatch.setenv("MRT_SWEEP_CAP", value)
        s = mrt_mod.Scene("cornellbox", device=-1)
        assert mrt_mod.debug_sweep_cap(s) == want
        s.close()
    monkeypatch.delenv("MRT_DIAG")                          # a diagnostic: ignored without MRT_DIAG=1
    s = mrt_mod.Scene("cornellbox", device=-1)
    assert mrt_mod.debug_sweep_cap(s) == default
    s.close()
