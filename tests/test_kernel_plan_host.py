"""The stack rule of csrc/kernel_plan.h (which LDS stack a renderer asks for and
which template STACK each kind of persistent kernel runs for it), printed by
tools/plan_check.cpp and compared with a restatement of the code it replaced:
the two rounding chains of mrt_renderer_create and the three if-chains of
kernels.hip (path_dispatch, dispatch, stream_grid / launch_stream), as they
stood before the plan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-renderer_amd", "csrc")

BOUNCE, PATH, STREAM = 0, 1, 2
# the STACK values each kind's kernel is instantiated with (negative: |STACK| LDS entries + global spill)
INSTANTIATED = {
    PATH: {-8, -12, -16, -32, 8, 12, 16, 24, 32},
    BOUNCE: {-8, -16, -32, 8, 12, 16, 24, 32},
    STREAM: {8, 12, 16, 24, 32},
}
OVERRIDES = [None, 8, 12, 16, 24, 32, 40]
NEEDS = range(1, 65)


def old_stack_entries(need, override):
    """mrt_renderer_create: the cap, MRT_STACK, the rounding, the spill variants' sizes."""
    cap = 16 if need <= 16 else (12 if need > 32 else 8)
    if override is not None:
        cap = max(8, override)
    want = min(need, cap)
    e = 8 if want <= 8 else 12 if want <= 12 else 16 if want <= 16 else 24 if want <= 24 else 32
    if need > e:
        e = 8 if e <= 8 else 12 if e <= 12 else 16 if e <= 16 else 32
    return e


def old_nonspill(e):
    return 8 if e <= 8 else 12 if e <= 12 else 16 if e <= 16 else 24 if e <= 24 else 32


def old_path_stack(need, e):
    """kernels.hip path_dispatch"""
    if need > e:
        return -8 if e <= 8 else -12 if e <= 12 else -16 if e <= 16 else -32
    return old_nonspill(e)


def old_bounce_stack(need, e):
    """kernels.hip dispatch: no -12"""
    if need > e:
        return -8 if e <= 8 else -16 if e <= 16 else -32
    return old_nonspill(e)


def old_stream_stack(need, e):
    """kernels.hip stream_ok (its stack part), then stream_grid / launch_stream; None: not supported"""
    if not (need <= e and e <= 32):
        return None
    return old_nonspill(e)


OLD = {PATH: old_path_stack, BOUNCE: old_bounce_stack, STREAM: old_stream_stack}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tools", "plan_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        kind, need, ov, entries, stack, spills, supported = (int(w) for w in line.split())
        rows[(kind, need, None if ov < 0 else ov)] = (entries, stack, bool(spills), bool(supported))
    return rows


def test_every_case_is_printed(printed):
    assert set(printed) == {(k, n, o) for k in (BOUNCE, PATH, STREAM) for n in NEEDS for o in OVERRIDES}


@pytest.mark.parametrize("kind", [BOUNCE, PATH, STREAM])
def test_rule_is_the_replaced_chains(printed, kind):
    for need in NEEDS:
        for ov in OVERRIDES:
            entries, stack, spills, supported = printed[(kind, need, ov)]
            want_entries = old_stack_entries(need, ov)
            want_stack = OLD[kind](need, want_entries)
            case = (kind, need, ov)
            assert entries == want_entries, case
            assert spills == (need > want_entries), case
            assert supported == (want_stack is not None), case
            if supported:
                assert stack == want_stack, case
                assert stack in INSTANTIATED[kind], case
                assert (stack < 0) == spills and abs(stack) >= entries, case
            else:
                assert stack == 0, case   # no variant: nothing to launch


def test_the_quirks(printed):
    """The cases the rule must keep: the per-bounce kernel runs -16 for "12, spilling" (the default
    of a tree deeper than 32); 24 entries that still spill become 32; the stream kernel never spills."""
    assert printed[(BOUNCE, 48, None)] == (12, -16, True, True)
    assert printed[(PATH, 48, None)] == (12, -12, True, True)
    assert printed[(PATH, 26, None)] == (8, -8, True, True)
    assert printed[(PATH, 40, 24)] == (32, -32, True, True)
    assert printed[(PATH, 30, 24)] == (32, 32, False, True)
    assert printed[(STREAM, 48, None)] == (12, 0, True, False)
    assert printed[(STREAM, 14, None)] == (16, 16, False, True)
    assert all(not sup for (k, _, _), (_, _, spills, sup) in printed.items() if k == STREAM and spills)
