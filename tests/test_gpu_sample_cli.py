"""exaRender --resample: the uniform-grid export of the CLI writes what the binding's Renderer.resample returns, byte for
byte, and reports how many grid points lie outside every region."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from common import ROOT, Case
from owlexabrick_amd import scenes

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")


def _grid_positions(lo, hi, dims):
    f = np.float32
    lo, hi = np.asarray(lo, f), np.asarray(hi, f)
    axes = [lo[k] + (np.arange(dims[k], dtype=f) + f(0.5)) * ((hi[k] - lo[k]) / f(dims[k])) for k in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(f)


@pytest.mark.parametrize("box", [None, "grown"], ids=["voxel-bounds", "grown-box"])
def test_exarender_resample_writes_the_bindings_bytes(box):
    scene = scenes.amr(levels=3, fields=2)
    R = Case(scene).hip_renderer()
    lo, hi = R.prep.voxel_bounds()
    dims = (23, 17, 9)
    args = []
    if box == "grown":
        ext = hi - lo
        lo, hi = (lo - 0.1 * ext).astype(np.float32), (hi + 0.1 * ext).astype(np.float32)
        args = ["--resample-box"] + [repr(float(v)) for v in lo] + [repr(float(v)) for v in hi]
    want = R.resample(lo, hi, dims, channel=1, fill=-7.0)
    _, _, st = R.samplePoints(_grid_positions(lo, hi, dims), channels=(1,))
    invalid = int((st < 0).sum())
    assert (invalid > 0) == (box == "grown")
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "amr")
        raw = os.path.join(d, "grid.raw")
        r = subprocess.run([EXE, cfg, "--resample", *map(str, dims), raw, "--resample-channel", "1", "--resample-fill", "-7",
                            "--frames", "0", *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(raw, dtype=np.float32)
    assert got.tobytes() == want.tobytes()
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("resample ")]
    assert len(line) == 1, r.stdout
    m = re.fullmatch(r"resample 23 17 9 box (\S+ ){6}channel 1 invalid (\d+)", line[0])
    assert m and int(m.group(2)) == invalid, line[0]
    assert "Avg. after" not in r.stdout                        # --frames 0: nothing rendered
