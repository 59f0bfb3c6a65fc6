"""The deferred sample epilogue of the cube march on the GPU (EXA_MARCH_DEFER, owlexabrick_amd/csrc/exa_kernels.hip): the cube
instantiations of the one-channel rope march shade a finished sample one brick visit late, between the issue of the next
visit's cell loads and their first use.  Every sample is still shaded and composited with the same operations on the same
values in the same order, so a frame is the same frame bit for bit as from the march headers (cube_records 0), whose kernels
keep the epilogue in place.  The method is tests/test_gpu_cube_records.py's: frames 0 and 1 of one handle with cube_records 0
and 1, RGBA8 and the accumulation buffer equal without a tolerance.  The cases are the places where a sample that waits can go
wrong: a ray that its waiting sample ends (its first one included) and the flush behind the loop, pops and walk bursts
between a sample and its epilogue, regions of another cell width in between, rays of no or one sample, the surfaces'
output path and the tile-major output of a shard.

The wide march is switched off (wide_march 0): in frames this small the tile-cost feedback of the first frame hands most tiles
to it, and it reads the march headers with either setting, so the frames that follow would compare it with itself."""
import numpy as np
import pytest

from common import band_xf, ramp_xf
from test_gpu_cube_records import EDGES, H, W, amr, assert_same, cube_case, frames_with, is_cube_scene

pytestmark = pytest.mark.gpu


def faint_xf():
    """the colour ramp at opacity 0.1 everywhere: times an opacity scale of 9.9 every sample is all but opaque"""
    xf = ramp_xf()
    xf[:, 3] = 0.1
    return xf


OPAQUE_SCALE = 9.9                    # 0.1 * 9.9 = 0.99 per unit step: 0.9 after a step of 0.5, 0.99 >= 0.98 after two


def slab(scene):
    """a slab one and a half finest cells thick across the middle of the volume, facing the camera (which looks down z)"""
    ext = np.asarray(scene.meta["extent"], dtype=np.float64)
    return ([0.0, 0.0, 0.5 * ext[2]], [float(ext[0]), float(ext[1]), 0.5 * ext[2] + 1.5])


CASES = {
    "opaque": lambda s: dict(xf=faint_xf(), opacity_scale=OPAQUE_SCALE),
    "band": lambda s: dict(xf=band_xf(), space_skipping=1),
    "dt2": lambda s: dict(dt=2.0),
    "dt03": lambda s: dict(dt=0.3),
    "clip": lambda s: dict(clip=slab(s)),
    "noskip": lambda s: dict(xf=band_xf(), space_skipping=0),
    "iso": lambda s: dict(iso=[(0.4, 0)]),
    "shard": lambda s: dict(),
}


def counters(R):
    """the counting variant's totals of frame 0 (it marches on the march headers, in the parent's order)"""
    R.updateFrameID(0)
    return R.renderStats()[1]


@pytest.mark.parametrize("grad", [0, 1], ids=["plain", "gradient"])
@pytest.mark.parametrize("kind", list(CASES))
@pytest.mark.parametrize("B", EDGES)
def test_deferred_epilogue_renders_the_same_frame_bit_for_bit(B, kind, grad):
    scene = amr(B)
    kw = CASES[kind](scene)
    case = cube_case(scene, grad=grad, **kw)
    R = case.hip_renderer()
    try:
        assert is_cube_scene(R) == int(np.log2(B))
        R.setOption("wide_march", 0)                            # every tile by the march under test, in every frame
        if kind == "shard":
            R.setShard(1, 3)                                    # tiles 1, 4, 7, ...: tile-major output
        base = frames_with(R, 0)
        cube = frames_with(R, 1)
        assert_same(base, cube, (B, kind, grad))
        acc = base[0][1]
        assert np.isfinite(acc).all() and (acc[..., :3] > 0).any(), "the frame shows the volume"
        if kind == "shard":
            assert base[0][0].ndim == 1 and base[0][0].size == 5 * 256
        if kind == "opaque":
            # rays end within their first samples: fewer samples than with the same TF at scale 1
            st = counters(R)
            xf = case.xfs[0]
            R.updateXF(0, xf[:, 3], xf[:, :3], case.xf_domains[0], 1.0)
            st1 = counters(R)
            print(f"samples at opacity scale {OPAQUE_SCALE}: {st['samples']}, at 1: {st1['samples']}")
            assert 0 < st["samples"] < st1["samples"], (st["samples"], st1["samples"])
        if kind == "band":
            # inactive regions between the segments: pops and walk bursts between a sample and its epilogue
            st = counters(R)
            print(f"segments {st['segments']} of {W * H} rays")
            assert st["segments"] > W * H, st["segments"]
    finally:
        R.close()
