"""exaRender --lic: the file holds the image that the binding's Renderer.lic returns for the same plane, channels, step, half
length and seed, byte for byte; a bad channel list and what the module refuses are errors."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import lic_ref as lr
from common import ROOT, Case
from owlexabrick_amd import scenes

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")


def test_exarender_lic_writes_the_bindings_bytes():
    scene = scenes.amr(levels=3, fields=4)
    R = Case(scene).hip_renderer()
    origin, du, dv, size = pl = lr.plane((3.0, 1.0, 6.0), (0.6, 0.1, 0.05), (-0.1, 1.0, 0.35), (67, 45))
    want = R.lic(pl, (1, 3, 0), 0.5, 9, seed=17)
    assert (want["count"] > 1).sum() > 1000 and (want["count"] == 0).any()
    args = [*(repr(float(c)) for v in (origin, du, dv) for c in v), *map(str, size), "0.5", "9"]      # o u v NU NV STEP HALFLENGTH
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "amr3")
        out = os.path.join(d, "cut.lic")
        r = subprocess.run([EXE, cfg, "--frames", "0", "--lic", "1,3,0", *args, out, "--lic-seed", "17"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        with open(out, "rb") as f:
            head = f.readline().decode()
            body = f.read()
        assert re.fullmatch(r"lic 67 45 channels 1 3 0 step 0\.5 halfLength 9 seed 17\n", head), head
        assert body == want["lic"].tobytes()
        assert (f"lic 67 45 channels 1 3 0 step 0.5 halfLength 9 seed 17 pixels_covered {int((want['count'] > 0).sum())} "
                f"samples {int(want['count'].sum())}") in r.stdout, r.stdout
        assert "Avg. after" not in r.stdout                    # --frames 0: nothing rendered
        # the default seed is 0
        r = subprocess.run([EXE, cfg, "--frames", "0", "--lic", "1,3,0", *args, out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        with open(out, "rb") as f:
            f.readline()
            assert f.read() == R.lic(pl, (1, 3, 0), 0.5, 9)["lic"].tobytes()
        for channels, tail, word in (("1,3", args, "--lic wants"), ("1;3;0", args, "--lic wants"), ("1,3,0,2", args, "--lic wants"),
                                     ("1,3,7", args, "exa_hip_lic"), ("1,3,0", args[:-1] + ["0"], "exa_hip_lic")):
            r = subprocess.run([EXE, cfg, "--frames", "0", "--lic", channels, *tail, out], capture_output=True, text=True, timeout=300)
            assert r.returncode != 0 and word in r.stderr + r.stdout, (channels, r.stderr)
    R.close()
