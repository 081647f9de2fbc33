"""CPU: the leaf tests' acceptance predicates in the walk's form and in the
sweep's short one (metal-renderer_amd/csrc/tri_accept.h) agree bit
for bit.

tools/tri_accept_model.cpp compiles the header twice — without contraction
(the precise build) and with std::fmaf where the fast build contracts, b1 + b2
as one fma with either of its products — and runs the cross product of special
values (±0, denormals, the neighbours of 0 and 1, ±inf, NaN) through both forms
of the range test and of the nearest rule, and through the occlusion rule
(occlusion_accepts, the one text of the shadow queries) against its written-out
form, then 1e6 random rays against triangles and their copies, many aimed at a
vertex or an edge.  Part 7 of
tools/walk_model.cpp runs the forms on its adversarial rays (origins inside and
on the faces of the record boxes, direction components 0, -0, ±1e-20) against
every triangle of the scene in both arithmetics.  Cap: 0 disagreements.

(Phase 1 reads no padded records: groups filled up with records no ray hits
were built, measured slower than whole groups followed by single records, and
removed — DESIGN §2.1t — so there is no padding whose keys or mask bits could
be checked.)"""
import os
import re
import subprocess

import pytest

import roomgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-renderer_amd", "csrc")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("tri_accept")
    out = {}
    for fma in (0, 1):
        out[fma] = str(d / f"tri_accept_model_{fma}")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-DMODEL_FMA={fma}", "-I" + CSRC,
                        os.path.join(ROOT, "tools", "tri_accept_model.cpp"), "-o", out[fma]], check=True)
    out["walk"] = str(d / "walk_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, os.path.join(ROOT, "tools", "walk_model.cpp"),
                    os.path.join(CSRC, "scene.cpp"), os.path.join(CSRC, "bvh.cpp"), "-o", out["walk"], "-lpthread"],
                   check=True)
    return out


def _numbers(line, *names):
    return [int(re.search(rf"\b{n} (\d+)", line).group(1)) for n in names]


@pytest.mark.parametrize("fma", [0, 1])
def test_special_values_and_random_triangles(models, fma):
    r = subprocess.run([models[fma], "1000000"], capture_output=True, text=True, check=True)
    line = r.stdout.strip()
    print(line)
    special, rand = line.split(" ; ")
    tests, bary, nearest, occlusion = _numbers(special, "tests", "bary", "nearest", "occlusion")
    assert tests >= 100000 and bary == 0 and nearest == 0 and occlusion == 0
    cases, tests, bary, nearest, state, occlusion = _numbers(rand, "cases", "tests", "bary", "nearest", "state", "occlusion")
    assert cases == 1000000 and tests >= 8 * cases and bary == 0 and nearest == 0 and state == 0 and occlusion == 0


@pytest.mark.parametrize("name", ["cornellbox", "plain-1", "wedge", "plain-4"])
def test_adversarial_rays(mrt_mod, models, tmp_path, name):
    path = mrt_mod.scene_path(name) if name == "cornellbox" else roomgen.room(name, roomgen.seeds(name)[0], tmp_path).path
    r = subprocess.run([models["walk"], path, "8"], capture_output=True, text=True, check=True)
    line = next(l for l in r.stdout.splitlines() if l.startswith("accept forms:"))
    print(line)
    rays, tests, bary, nearest = _numbers(line, "rays", "tests", "bary", "nearest")
    assert rays >= 2000 and tests >= 20 * rays and bary == 0 and nearest == 0

