"""The owning types of csrc/hip_handles.h (DevBuf, Event, Stream, PinnedBuf), compiled with g++ against
tools/hip_stub.cpp, which stands in for HIP and counts what is live: tools/handles_check.cpp prints one
line per case, compared here with what the types promise.  "live=E/S/P/D": live events / streams /
pinned blocks / device blocks; "bad": releases of something not live (a second release, a borrowed
handle) up to that line."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-renderer_amd", "csrc")
TOOLS = os.path.join(ROOT, "tools")

SLOTS = 8
AGGREGATE_CALLS = 1 + SLOTS + 12 + 2 + 1 + 1   # streams, ring events, two pinned (one mapped: two calls), image


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("handles") / "handles_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC,
                    "-o", exe, os.path.join(TOOLS, "handles_check.cpp"), os.path.join(TOOLS, "hip_stub.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr   # nothing live at its end, no bad release
    lines = {}
    for line in run.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "aggregate":
            k, _, rest = rest.partition(" ")
            name = "aggregate " + k
        assert name not in lines, name
        lines[name] = rest
    return lines


def test_no_release_of_anything_not_live(printed):
    assert all(rest.endswith("bad=0") for rest in printed.values()), printed


def test_moves_leave_one_owner(printed):
    assert printed["event_move_construct"] == "from_empty=1 to_same=1 live=1/0/0/0 bad=0"
    assert printed["event_move_assign"] == "from_empty=1 to_same=1 live=1/0/0/0 bad=0"   # the target's own event went
    assert printed["event_self_assign"] == "live=1/0/0/0 bad=0"
    assert printed["event_scope_end"] == "live=0/0/0/0 bad=0"
    assert printed["stream_move"] == "from_empty=1 to_same=1 live=0/1/0/0 bad=0"
    assert printed["devbuf_move_construct"] == "from_empty=1 to_same=1 bytes=100 live=0/0/0/1 bad=0"
    assert printed["devbuf_move_assign"] == "from_empty=1 to_same=1 bytes=100 live=0/0/0/1 bad=0"
    assert printed["devbuf_alloc_zero"] == "empty=1 bytes=0 live=0/0/0/0 bad=0"
    assert printed["devbuf_scope_end"] == "live=0/0/0/0 bad=0"
    assert printed["pinned_move"] == "from_empty=1 bytes=2000 live=0/0/1/0 bad=0"
    assert printed["pinned_scope_end"] == "live=0/0/0/0 bad=0"


def test_borrow_never_destroys(printed):
    assert printed["stream_borrow"] == "same=1 from_empty=1 live=0/1/0/0 bad=0"
    assert printed["stream_borrow_reset"] == "live=0/1/0/0 bad=0"
    assert printed["stream_borrow_over_own"] == "live=0/1/0/0 bad=0"   # the stream it had created went, the lent one stays
    assert printed["stream_scope_end"] == "live=0/0/0/0 bad=0"         # destroyed once, by its owner


def test_ensure_creates_once(printed):
    assert printed["event_ensure"] == "creates=1 same=1 live=1/0/0/0 bad=0"
    assert printed["event_ensure_scope_end"] == "live=0/0/0/0 bad=0"


def test_reserve_grows_only_and_fails_empty(printed):
    assert printed["pinned_reserve"] == "bytes=1000 mapped=1 device_set=1 live=0/0/1/0 bad=0"
    assert printed["pinned_reserve_smaller"] == "bytes=1000 same=1 calls=0 live=0/0/1/0 bad=0"
    assert printed["pinned_reserve_grow"] == "bytes=2000 default=1 device_set=0 live=0/0/1/0 bad=0"
    assert printed["pinned_failed_grow"] == "failed=1 empty=1 bytes=0 live=0/0/0/0 bad=0"
    assert printed["pinned_failed_map"] == "failed=1 empty=1 bytes=0 live=0/0/0/0 bad=0"


def test_failed_create_of_a_renderer_shaped_aggregate_leaks_nothing(printed):
    ks = [k for k in range(1, AGGREGATE_CALLS + 2)]
    assert sorted(int(n.split("=")[1]) for n in printed if n.startswith("aggregate ")) == ks
    objects = 1 + SLOTS + 12 + 2 + 1
    for k in ks:
        failed = k <= AGGREGATE_CALLS
        # what stood when create returned: one object per call before the failing one; the mapped
        # buffer is two calls (calls 22 and 23 with 8 slots) and gone again if its second fails
        first_pinned = 1 + SLOTS + 12 + 1
        made = objects if not failed else (k - 1 if k <= first_pinned else k - 2)
        assert printed[f"aggregate k={k}"] == f"failed={int(failed)} made={made} live=0/0/0/0 bad=0", k
