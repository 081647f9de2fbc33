"""CPU: the Python binding (metal-renderer_amd/mrt.py) against include/mrt.h —
every entry point's name and argument types, every struct's fields, types and
size, every mirrored constant, and the ABI version.  The comparison itself is
tests/abi_header.py; it is shown to see each kind of edit on a doctored header.

Adding an entry point: its prototype in the header, one line in mrt.py's table;
this file then says what else is missing."""
import ctypes
import os

import pytest

from abi_header import Header, mismatches, struct_classes
from adaptive_model import TILE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI_VERSION = 9      # written once: a bump is a deliberate edit here, in the header and in the library
SIZES = {"mrt_scene_desc": 56, "mrt_scene_info": 608, "mrt_accel_desc": 48, "mrt_accel_info": 40, "mrt_camera": 60,
         "mrt_denoise_params": 16, "mrt_reproject_params": 12, "mrt_svgf_params": 20, "mrt_firefly_params": 20,
         "mrt_adaptive_params": 4, "mrt_error_summary": 32, "mrt_converge_params": 32, "mrt_renderer_desc": 64,
         "mrt_stats": 160, "mrt_refine_stats": 32, "mrt_converge_result": 80}


@pytest.fixture(scope="module")
def header_text():
    with open(os.path.join(ROOT, "include", "mrt.h")) as f:
        return f.read()


def test_binding_matches_the_header(mrt_mod, header_text):
    h = Header(header_text)
    assert len(h.prototypes) == len(mrt_mod._ABI) >= 127 and len(h.structs) == 16   # the parse saw the header
    assert mismatches(header_text, mrt_mod) == []


def test_struct_sizes(mrt_mod, header_text):
    classes = struct_classes(mrt_mod)
    assert set(classes) == set(SIZES) == set(Header(header_text).structs)
    assert {n: ctypes.sizeof(c) for n, c in classes.items()} == SIZES


def test_library_exports_every_entry_of_the_table(mrt_mod, header_text):
    plain = ctypes.CDLL(mrt_mod.LIB_PATH)
    assert not [n for n in mrt_mod.EXPORTED if not hasattr(plain, n)]
    bound = mrt_mod.lib()
    for n, args in mrt_mod._ABI.items():
        fn = getattr(bound, n)
        assert fn.argtypes is not None and list(fn.argtypes) == args, n      # bound with the table's signature
        assert fn.restype is (ctypes.c_char_p if n == "mrt_last_error" else ctypes.c_int), n
    assert Header(header_text).defines["MRT_ABI_VERSION"] == bound.mrt_abi_version() == ABI_VERSION


def test_wrappers_and_exact_values(mrt_mod):
    """What the per-feature symbol tests asserted beyond the header check."""
    for name in ("error_estimate", "converge", "read_tile_error"):
        assert callable(getattr(mrt_mod.Renderer, name))
    assert callable(mrt_mod.tile_error) and callable(mrt_mod.tile_threshold)
    assert mrt_mod.REFINE_SEED_XOR == 0x9E3779B97F4A7C15
    assert mrt_mod.FLAG_MOMENTS == 32 and mrt_mod.DISPLAY_RESOLVED == 8
    assert mrt_mod.TILE == TILE == 64


# one edit of the real header each: (what, text in the header, its replacement, the entry the report must name)
EDITS = [
    ("argument uint32_t -> uint64_t", "int mrt_renderer_resize(mrt_renderer* r, uint32_t width,",
     "int mrt_renderer_resize(mrt_renderer* r, uint64_t width,", "mrt_renderer_resize: argument 1 (width)"),
    ("argument float -> uint32_t", "uint32_t flags, float compare_scale, void* stream);",
     "uint32_t flags, uint32_t compare_scale, void* stream);", "mrt_display: argument 6 (compare_scale)"),
    ("argument dropped", "int mrt_renderer_draw_n(mrt_renderer* r, uint32_t n);", "int mrt_renderer_draw_n(mrt_renderer* r);",
     "mrt_renderer_draw_n: 1 parameters in the header, 2 in the table"),
    ("prototype removed", "int mrt_renderer_sync(mrt_renderer* r);", "", "mrt_renderer_sync: in the table, not declared"),
    ("prototype added", "int mrt_renderer_sync(mrt_renderer* r);",
     "int mrt_renderer_sync(mrt_renderer* r);\nint mrt_renderer_sync_twice(mrt_renderer* r);",
     "mrt_renderer_sync_twice: declared in the header, not in the table"),
    ("field renamed", "float sigma_color; ", "float sigma_colour; ", "mrt_denoise_params: fields"),
    ("field float -> uint32_t", "float k; ", "uint32_t k; ", "mrt_firefly_params.k: is c_float, the header wants c_uint"),
    ("array dimensions swapped", "float occluder_plane[8][4];", "float occluder_plane[4][8];",
     "mrt_scene_info.occluder_plane: is c_float[8][4], the header wants c_float[4][8]"),
    ("#define value changed", "#define MRT_FLAG_MOMENTS 32u", "#define MRT_FLAG_MOMENTS 64u", "FLAG_MOMENTS: 32 here, MRT_FLAG_MOMENTS is 64"),
    ("status value changed", "MRT_ERR_COMM = -6", "MRT_ERR_COMM = -7", "ERR_COMM: -6 here, MRT_ERR_COMM is -7"),
]


@pytest.mark.parametrize("what,old,new,entry", EDITS, ids=[e[0] for e in EDITS])
def test_comparator_reports_a_doctored_header(mrt_mod, header_text, what, old, new, entry):
    assert header_text.count(old) == 1, what
    found = mismatches(header_text.replace(old, new), mrt_mod)
    assert len(found) == 1 and found[0].startswith(entry), found
