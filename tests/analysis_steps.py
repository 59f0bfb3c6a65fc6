"""What the GPU tests of the calls that read the field outside a frame share (test_gpu_sample, test_gpu_isomesh,
test_gpu_histogram, test_gpu_streamlines, test_gpu_project): float bits, the scene without its kd tree, the multi-device
handle with a repeated device, and the one list of what a frame sets and a call's bytes must not depend on."""
import numpy as np

from owlexabrick_amd import binding


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def without_kd_tree(case_or_prep):
    """drops the region kd-tree of a Prep's scene, or has a Case drop it from the Prep it makes; returns its argument"""
    def drop_kd_tree(prep):
        prep.scene.kdNodes = None
        prep.scene.numKdNodes = 0

    if isinstance(case_or_prep, binding.Prep):
        drop_kd_tree(case_or_prep)
    else:
        case_or_prep.prep_edit = drop_kd_tree
    return case_or_prep


def multi_handle(R, form=None):
    """a multi-device handle on R's scene that names device 0 twice, with the basis form set where one is given"""
    M = binding.Renderer(R.prep, devices=[0, 0])
    if form is not None:
        M.setOption("basis_form", form)
    return M


def frame_perturbations(case, R):
    """Changes, one after the other, what a frame sets on the renderer R of `case` (a 32 x 32 frame), renders where a frame is
    what applies the change, and yields a label after each: the caller repeats its call and compares the bytes.  The changes
    accumulate, except that accel goes back to 1 behind its step."""
    for c in range(len(case.scene.fields)):                     # every region inactive
        R.updateXF(c, np.zeros(128, np.float32), case.xfs[c][:, :3], case.xf_domains[c], 1.0)
    R.render()
    assert not R.readActivity(0).any()
    yield "inactive TF"
    R.updateIsoValues([0.5, 0.3], [0, 1], [1, 1])
    R.render()
    yield "iso values"
    R.updateCamera([1, 2, 3], [0, 0, -1], [0.01, 0, 0], [0, 0.01, 0])
    R.render()
    yield "another camera in the frame state"
    for walk in (1, 2):
        R.setOption("walk", walk)
        R.render()
        yield f"walk {walk}"
    R.setOption("accel", 0)
    R.render()
    yield "accel 0"
    R.setOption("accel", 1)
    R.setOption("interleave", 0)
    R.render()
    yield "interleave 0"
    R.setOption("brick_order", 1)                               # pending: the call applies it
    yield "brick_order 1 before a frame"
    R.render()
    yield "brick_order 1 after a frame"
    R.setOption("brick_order", 0)
    R.render()
    R.setOption("brick_order", 1)
    R.render()                                                  # applied by the frame this time
    yield "brick_order 1 applied by a frame"
    R.setOption("brick_order", 0)                               # pending again
    yield "brick_order back to 0"
