"""exaRender --raycast: the CLI casts along the frame's own camera through the pixel centres — world space, unit directions —
and writes a text line and seven raw arrays (t, position, value, gradient, index, side, crossings); the arrays are the
binding's Renderer.raycast_iso with the camera the CLI prints, bit for bit."""
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
ARRAYS = (("t", "<f4", 1), ("position", "<f4", 3), ("value", "<f4", 1), ("gradient", "<f4", 3), ("index", "<i4", 1),
          ("side", "<i4", 1), ("crossings", "<u4", 1))


@pytest.mark.parametrize("channel,iso,refine", [(0, 0.5, 8), (1, 0.625, 0)])
def test_exarender_raycast_writes_the_bindings_arrays(channel, iso, refine):
    scene = scenes.amr(levels=3, fields=2)
    W, H, dt, n = 37, 21, 0.75, 160
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "amr")
        out = os.path.join(d, "amr.hit")
        r = subprocess.run([EXE, cfg, "--size", str(W), str(H), "--raycast", str(channel), str(iso), str(dt), str(n), str(refine), out,
                            "--frames", "0"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        with open(out, "rb") as f:
            header = f.readline().decode()
            raw = f.read()
    assert header == f"raycast {W} {H} channel {channel} iso {iso} dt {dt} samples {n} refine {refine}\n"
    assert len(raw) == 4 * W * H * sum(c for _, _, c in ARRAYS)
    got, at = {}, 0
    for name, t, c in ARRAYS:
        got[name] = np.frombuffer(raw, dtype=t, count=W * H * c, offset=at).reshape((H, W) + ((3,) if c == 3 else ()))
        at += 4 * W * H * c
    cam = [ln for ln in r.stdout.splitlines() if ln.startswith("camera ")]
    assert len(cam) == 1, r.stdout
    c = np.array([np.float32(x) for x in cam[0].split()[1:]], dtype=np.float32).reshape(4, 3)      # printed with %.9g: round-trips
    R = Case(scene, W=W, H=H).hip_renderer()
    zero = (0, 0, 0)
    want = R.raycast_iso(c[0], zero, zero, c[1], c[2], c[3], (W, H), 0.0, dt, n, iso=iso, refine=refine, channel=channel, world=True,
                         normalize=True)
    hits = int((want["index"] >= 0).sum())
    assert hits > 50
    for name, _, _ in ARRAYS:
        assert got[name].dtype.itemsize == want[name].dtype.itemsize and got[name].tobytes() == np.ascontiguousarray(want[name]).tobytes(), name
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("raycast ")]
    assert len(line) == 1, r.stdout
    m = re.fullmatch(rf"raycast {W} {H} channel {channel} iso {iso} dt 0\.75 samples {n} refine {refine} pixels_hit (\d+)", line[0])
    assert m and int(m.group(1)) == hits, line[0]
    assert "Avg. after" not in r.stdout                        # --frames 0: nothing rendered
    R.close()
