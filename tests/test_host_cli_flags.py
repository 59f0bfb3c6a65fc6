"""exaRender's flag errors, word for word: every "missing ..." and "wants ..." text of the command line, which fire before the
config is read (so the config named here need not exist and nothing touches a GPU)."""
import os
import subprocess

import pytest

from common import ROOT

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")
CFG = "no_such_config.exa"

# flag -> how many numbers it reads before anything else it takes: one fewer gives "missing value after FLAG"
NUMBERS = {
    "--size": 2, "-win": 2, "--camera": 9, "--fov": 1, "--dt": 1, "--xf-scale": 1, "--range": 2, "--isovals": 2, "--isochans": 2,
    "--contourplane": 4, "--contourchan": 1, "--clip-box": 6, "--ao-length": 1, "--gradientShadingDVR": 1,
    "--gradientShadingISO": 1, "--frames": 1, "--gpus": 1, "--resample": 3, "--resample-box": 6, "--resample-channel": 1,
    "--resample-fill": 1, "--isomesh": 4, "--isomesh-box": 6, "--isomesh-channel": 1, "--isolines": 12, "--lic-seed": 1,
    "--regions": 5, "--basins": 6, "--regions-box": 6, "--histogram": 1, "--histogram-channel": 1, "--histogram-range": 2,
    "--histogram-box": 6, "--streamlines-channels": 3, "--project": 3, "--raycast": 5,
}
# the flags that read a word first and numbers after it: (flag, the words, how many numbers follow)
WORD_THEN_NUMBERS = [("--lic", ["0,1,2"], 13), ("--critical", ["0,1,2"], 11), ("--ftle", ["0,1,2"], 11), ("--derived", ["q"], 3),
                     ("--streamlines", ["seeds.txt"], 2), ("--surface", ["iso", "0"], 2)]

PLANE = ["0", "0", "0", "1", "0", "0", "0", "1", "0", "4", "4"]      # o u v NU NV
BOX_DIMS = ["0", "0", "0", "1", "1", "1", "2", "2", "2"]           # l u NX NY NZ
C3 = "wants three comma-separated channels C0,C1,C2"
DEVICES = "--devices wants a comma-separated list of device indices"
DERIVED = "--derived wants speed, divergence, vorticity, vorticity_magnitude, q, helicity or a number, not "
CONFLICT = "--derived takes its three channels itself: --resample-channel / --isomesh-channel do not go with it"

TABLE = [(["--bogus"], "unknown flag --bogus"), ([], None)]           # None: no config at all, the usage line (CFG left out)
TABLE += [([flag] + ["1"] * (n - 1), "missing value after " + flag) for flag, n in NUMBERS.items()]
TABLE += [([flag] + words + ["1"] * (n - 1), "missing value after " + flag) for flag, words, n in WORD_THEN_NUMBERS]
TABLE += [
    (["--xf"], "missing file after --xf"),
    (["-o"], "missing file after -o"),
    (["--devices"], "missing list after --devices"),
    (["--devices", "a"], DEVICES), (["--devices", "0;1"], DEVICES), (["--devices", "0,"], DEVICES), (["--devices", "-1"], DEVICES),
    (["--devices", "1024"], DEVICES), (["--devices", "0,,1"], DEVICES), (["--devices", ""], DEVICES),
    (["--option"], "missing key=value after --option"),
    (["--option", "walk"], "--option wants key=integer"), (["--option", "=2"], "--option wants key=integer"),
    (["--option", "walk=two"], "--option wants key=integer"), (["--option", "walk="], "--option wants key=integer"),
    (["--resample", "2", "2", "2"], "missing file after --resample NX NY NZ"),
    (["--isomesh", "0.5", "2", "2", "2"], "missing file after --isomesh ISO NX NY NZ"),
    (["--isolines", "0"] + PLANE, "missing levels and file after --isolines CHANNEL o u v NU NV"),
    (["--isolines", "0"] + PLANE + ["0.5"], "missing levels and file after --isolines CHANNEL o u v NU NV"),
    (["--isolines", "0"] + PLANE + ["0.5;0.6", "o.isolines"], "--isolines wants a comma-separated list of levels"),
    (["--isolines", "0"] + PLANE + ["0.5,,0.6", "o.isolines"], "--isolines wants a comma-separated list of levels"),
    (["--isolines", "0"] + PLANE + ["high", "o.isolines"], "--isolines wants a comma-separated list of levels"),
    # an empty list of levels is no parse error: the next thing to fail is the config
    (["--isolines", "0"] + PLANE + ["", "o.isolines"], "error in opening config file '" + CFG + "'"),
    (["--lic"], "missing channels after --lic"),
    (["--lic", "0,1,2x"], "--lic " + C3), (["--lic", "0,1"], "--lic " + C3), (["--lic", "0 1 2"], "--lic " + C3),
    (["--lic", "0,1,2"] + PLANE + ["0.5", "20"], "missing file after --lic C0,C1,C2 o u v NU NV STEP HALFLENGTH"),
    (["--critical"], "missing channels after --critical"),
    (["--critical", "0,1,2x"], "--critical " + C3), (["--critical", "0,1"], "--critical " + C3),
    (["--critical", "0,1,2"] + BOX_DIMS + ["8", "0.001"], "missing file after --critical C0,C1,C2 l u NX NY NZ ITERATIONS TOLERANCE"),
    (["--ftle"], "missing channels after --ftle"),
    (["--ftle", "0,1,2x"], "--ftle " + C3), (["--ftle", "0,1"], "--ftle " + C3),
    (["--ftle", "0,1,2"] + BOX_DIMS + ["0.5", "20"], "missing direction and file after --ftle C0,C1,C2 l u NX NY NZ STEP NUMSTEPS"),
    (["--ftle", "0,1,2"] + BOX_DIMS + ["0.5", "20", "fwd"], "missing direction and file after --ftle C0,C1,C2 l u NX NY NZ STEP NUMSTEPS"),
    (["--ftle", "0,1,2"] + BOX_DIMS + ["0.5", "20", "forward", "o.ftle"], "--ftle wants the direction fwd or bwd"),
    (["--ftle", "0,1,2"] + BOX_DIMS + ["0.5", "20", "", "o.ftle"], "--ftle wants the direction fwd or bwd"),
    (["--regions", "0", "0.5", "2", "2", "2"], "missing file after --regions CHANNEL ISO NX NY NZ"),
    (["--basins", "0", "0.5", "0.1", "2", "2", "2"], "missing file after --basins CHANNEL ISO MINDEPTH NX NY NZ"),
    (["--derived"], "missing quantity after --derived"),
    (["--derived", "curl", "0", "1", "2"], DERIVED + "curl"), (["--derived", "-1", "0", "1", "2"], DERIVED + "-1"),
    (["--derived", "4x", "0", "1", "2"], DERIVED + "4x"), (["--derived", "", "0", "1", "2"], DERIVED),
    (["--derived", "q", "0", "1", "2", "--resample-channel", "1"], CONFLICT),
    (["--resample-channel", "1", "--derived", "q", "0", "1", "2"], CONFLICT),
    (["--derived", "4", "0", "1", "2", "--isomesh-channel", "0"], CONFLICT),
    (["--histogram", "16"], "missing file after --histogram BINS"),
    (["--streamlines"], "missing seed file after --streamlines"),
    (["--streamlines", "seeds.txt", "0.5", "10"], "missing file after --streamlines SEEDS.txt STEP MAXSTEPS"),
    (["--project", "0", "0.5", "10"], "missing file after --project CHANNEL DT NSAMPLES"),
    (["--raycast", "0", "0.5", "0.5", "10", "4"], "missing file after --raycast CHANNEL ISO DT NSAMPLES REFINE"),
    (["--surface"], "missing mesh and channels after --surface"),
    (["--surface", "iso"], "missing mesh and channels after --surface"),
    (["--surface", "iso", "1,,2", "0.5", "4", "o.surf"], "--surface: channels are C0[,C1,C2,C3]"),
    (["--surface", "iso", "a", "0.5", "4", "o.surf"], "--surface: channels are C0[,C1,C2,C3]"),
    (["--surface", "iso", "0;1", "0.5", "4", "o.surf"], "--surface: channels are C0[,C1,C2,C3]"),
    (["--surface", "iso", "0,1,2", "0.5", "4"], "missing file after --surface MESH CHANNELS SPACING MAXN"),
]


@pytest.mark.parametrize("tail,text", TABLE, ids=[" ".join(t) or "nothing" for t, _ in TABLE])
def test_flag_error_text(tail, text):
    args = [CFG] + tail if text is not None else tail
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert r.stderr == "Fatal error " + (text if text is not None else "usage: exaRender cfg.exa [flags]") + "\n"
    assert r.stdout == ""
