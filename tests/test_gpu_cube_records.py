"""The cube records on the GPU (option cube_records, owlexabrick_amd/csrc/exa_cube.h): in a scene whose bricks are all cubes
of one power-of-two edge the one-channel 32-bit rope march reads 16-byte brick records and takes the edge as a kernel argument.
The same integers and floats enter every address and every float operation as from the 32-byte march headers, so a frame
is the same frame bit for bit: every case renders with cube_records 0 and 1 on one handle and compares the RGBA8 frame and
the accumulation buffer for equality, without a tolerance.  One case per scene holds the cube path against the oracle with
the comparison and the bounds of the shipped defaults (tests/common.py, tests/test_gpu_parity.py)."""
import numpy as np
import pytest

import probe_sets as ps
from common import MAX_ULP_SHIPPED, ULP_P999_SHIPPED, Case, compare, error_profile_line
from owlexabrick_amd import binding, scenes

pytestmark = pytest.mark.gpu

W, H = 72, 40                       # 5 x 3 tiles of 16 x 16, the last column and row partial
EDGES = [2, 4, 8]
_scenes = {}


def amr(B):
    """procedural AMR scene of B^3 blocks, three levels (made once per edge; nothing changes it)"""
    if B not in _scenes:
        _scenes[B] = scenes.amr(B=B, levels=3)
        assert 30 <= len(_scenes[B].bricks7) <= 600, len(_scenes[B].bricks7)
    return _scenes[B]


def frames_with(R, setting, shard=None):
    """frames 0 and 1 of the handle with cube_records = setting: [(rgba8, accum)] (frame 1 adds to frame 0's accumulation)"""
    R.setOption("cube_records", setting)
    out = []
    for frameID in (0, 1):
        R.updateFrameID(frameID)
        rgba = R.render()
        out.append((np.array(rgba, copy=True), R.readAccum().copy()))
    return out


def assert_same(a, b, what):
    for f, ((rgba_a, acc_a), (rgba_b, acc_b)) in enumerate(zip(a, b)):
        assert np.array_equal(rgba_a, rgba_b), (what, "rgba8 of frame", f, int((rgba_a != rgba_b).sum()))
        assert np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32)), (what, "accumulation of frame", f)


def cube_case(scene, **kw):
    """the case on the rope walk (accel 2) with the shipped defaults otherwise: the frame that takes the cube instantiation"""
    return Case(scene, W=W, H=H, accel=2, **kw)


def is_cube_scene(R):
    return binding.cube_records(R.prep.bricks(), R.prep.leaflist())[0]


KINDS = ["plain", "gradient", "iso", "iso-gradient", "shard", "translated", "brick_order"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", EDGES)
def test_frames_are_bit_identical_with_and_without_cube_records(B, kind):
    scene = amr(B)
    kw = {}
    if kind in ("gradient", "iso-gradient", "shard"):
        kw["grad"] = 1
    if kind in ("iso", "iso-gradient"):
        kw["iso"] = [(0.4, 0)]                                  # one iso-surface: the SURF instantiations
    if kind == "translated":
        ext = np.asarray(scene.meta["extent"], dtype=np.int64)
        scene = ps.translated(scene, tuple(int(-e) for e in ext))       # every lower corner negative, the upper corner at 0
        assert np.asarray(scene.bricks7)[:, 3:6].max() < 0
    R = cube_case(scene, **kw).hip_renderer()
    try:
        assert is_cube_scene(R) == int(np.log2(B))
        if kind == "shard":
            R.setShard(1, 3)                                    # tiles 1, 4, 7, ...: tile-major output
        base = frames_with(R, 0)
        cube = frames_with(R, 1)
        assert_same(base, cube, (B, kind))
        acc = base[0][1]
        assert np.isfinite(acc).all() and (acc[..., :3] > 0).any(), "the frame shows the volume"
        if kind == "shard":
            assert base[0][0].ndim == 1 and base[0][0].size == 5 * 256
        if kind == "brick_order":
            R.setOption("brick_order", 1)                       # the cells re-laid: begin of every record patched on the device
            assert_same(base, frames_with(R, 1), (B, kind, "cube records, Morton order"))
            assert_same(base, frames_with(R, 0), (B, kind, "march headers, Morton order"))
            R.setOption("brick_order", 0)                       # ... and back
            assert_same(base, frames_with(R, 1), (B, kind, "cube records, uploaded order again"))
    finally:
        R.close()


def test_mixed_brick_sizes_render_from_the_march_headers_with_either_setting():
    """ex4 has 4^3 and 2^3 bricks: no cube scene, nothing is built, and the option changes nothing"""
    R = cube_case(scenes.example("ex4"), grad=1).hip_renderer()
    try:
        assert is_cube_scene(R) == 0
        base = frames_with(R, 0)
        assert_same(base, frames_with(R, 1), "ex4")
        assert (base[0][1][..., :3] > 0).any()
    finally:
        R.close()


@pytest.mark.parametrize("B", EDGES)
def test_cube_path_matches_the_oracle(B):
    """the shipped kernel on the cube records (not the counting variant, which keeps the march headers) against the oracle:
    the comparison and the bounds tests/test_gpu_parity.py holds the shipped defaults to"""
    case = cube_case(amr(B), grad=1)
    o = case.run_oracle()
    R = case.hip_renderer()
    try:
        assert is_cube_scene(R) == int(np.log2(B))
        R.setOption("cube_records", 1)
        R.updateFrameID(0)
        rgba = R.render()
        h = (rgba, R.readAccum(), None)
    finally:
        R.close()
    r = compare(o, h, f"cube records, amr B={B}")
    print(error_profile_line(r))
    assert r["flips_ok"] and r["rgba_bad"] <= 3 * r["flip_pixels"], r
    assert r["max_ulp"] <= MAX_ULP_SHIPPED and r["ulp_p999"] <= ULP_P999_SHIPPED, r
