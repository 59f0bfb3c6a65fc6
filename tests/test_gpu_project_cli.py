"""exaRender --project: the CLI projects along the frame's own camera through the pixel centres — world space, unit
directions — and writes a text line and four raw planes (sum*dt as float32, count, max, min); the planes are the binding's
Renderer.project with the camera the CLI prints, bit for bit."""
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


@pytest.mark.parametrize("channel", [0, 1])
def test_exarender_project_writes_the_bindings_planes(channel):
    scene = scenes.amr(levels=3, fields=2)
    W, H, dt, n = 37, 21, 0.75, 160
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "amr")
        out = os.path.join(d, "amr.prj")
        r = subprocess.run([EXE, cfg, "--size", str(W), str(H), "--project", str(channel), str(dt), str(n), out, "--frames", "0"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        with open(out, "rb") as f:
            header = f.readline().decode()
            raw = f.read()
    assert header == f"project {W} {H} channel {channel} dt {dt} samples {n}\n"
    assert len(raw) == 4 * 4 * W * H
    planes = [np.frombuffer(raw, dtype=t, count=W * H, offset=4 * W * H * k).reshape(H, W)
              for k, t in enumerate(("<f4", "<u4", "<f4", "<f4"))]
    cam = [ln for ln in r.stdout.splitlines() if ln.startswith("camera ")]
    assert len(cam) == 1, r.stdout
    c = np.array([np.float32(x) for x in cam[0].split()[1:]], dtype=np.float32).reshape(4, 3)      # printed with %.9g: round-trips
    R = Case(scene, W=W, H=H).hip_renderer()
    zero = (0, 0, 0)
    want = R.project(c[0], zero, zero, c[1], c[2], c[3], (W, H), 0.0, dt, n, channel=channel, world=True, normalize=True)
    assert (want["count"] > 0).sum() > 50
    integral = (want["sum"] * np.float64(np.float32(dt))).astype(np.float32)
    for got, ref, name in zip(planes, (integral, want["count"], want["max"], want["min"]), ("integral", "count", "max", "min")):
        assert got.dtype.itemsize == ref.dtype.itemsize and got.tobytes() == np.ascontiguousarray(ref).tobytes(), name
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("project ")]
    assert len(line) == 1, r.stdout
    m = re.fullmatch(rf"project {W} {H} channel {channel} dt 0\.75 samples {n} pixels_hit (\d+)", line[0])
    assert m and int(m.group(1)) == int((want["count"] > 0).sum()), line[0]
    assert "Avg. after" not in r.stdout                        # --frames 0: nothing rendered
    R.close()
