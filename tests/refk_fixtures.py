"""The fixtures of tests/golden/make_reference_kernel_goldens.py -- the outputs of the reference's own stage kernels run
on the host -- as the CPU test (tests/test_reference_goldens.py, the oracle) and the GPU test
(tests/test_gpu_reference_goldens.py, the kernels) read them.  Only tests/golden/ is read here."""
from __future__ import annotations

import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAMERAS = ("tiny", "small")
STRIDES = {"tiny": (1, 3, 16), "small": (4, 5, 25)}
CASES = [(c, s) for c in CAMERAS for s in STRIDES[c]]
TAGS = ("3dof", "6dof")
DEPTH_FACTOR = 100.0  # rendered centimetres -> metres


def case_id(cs):
    return f"{cs[0]}-s{cs[1]}"


@functools.lru_cache(maxsize=None)
def load(name):
    """The arrays of tests/golden/<name>.npz, read-only."""
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def raster(cam, tag):
    return load(f"refk_raster_{cam}_{tag}")


def cloud(cam, stride):
    return load(f"refk_cloud_{cam}_s{stride}")


def observed(cam):
    return load(f"refk_observed_{cam}")


def camera(fx):
    """(fx, fy, cx, cy) as Python floats, from a fixture's `camera`."""
    return tuple(float(v) for v in fx["camera"])


def dc_index(dc_mask):
    """result_dc_index from the stored stride mask: its exclusive scan in pose / row / column order (the generator
    asserts that this gives the reference's array back)."""
    flat = dc_mask.reshape(-1).astype(np.int64)
    return (np.cumsum(flat) - flat).astype(np.int32).reshape(dc_mask.shape)


def bits(a):
    """An array's bytes as unsigned integers, for comparisons that tell -0.0 from 0.0 and NaNs apart."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}.get(a.dtype.itemsize, np.uint8))


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} differ; first at {tuple(bad[0])}: got " \
                          f"{got[tuple(bad[0])]!r}, reference {want[tuple(bad[0])]!r}"


@functools.lru_cache(maxsize=None)
def observation(cam, stride):
    """The observed cloud of a case as the evaluation takes it: (xyz (O, 3), label (O,), rgb (O, 3)) in the order of the
    fixture, and label-sorted (stable) with the segments' starts and ends, as the oracle takes it."""
    c = cloud(cam, stride)
    xyz, lab = np.ascontiguousarray(c["obs_xyz"]), np.ascontiguousarray(c["obs_label"])
    rgb = np.ascontiguousarray(c["obs_color"].T)
    order = np.argsort(lab, kind="stable")
    slab = lab[order]
    start = np.array([np.searchsorted(slab, L, "left") for L in range(2)], np.int32)
    end = np.array([np.searchsorted(slab, L, "right") for L in range(2)], np.int32)
    return dict(xyz=xyz, label=lab, rgb=rgb, order=order, sorted_xyz=np.ascontiguousarray(xyz[order]),
                sorted_rgb=np.ascontiguousarray(rgb[order]), label_start=start, label_end=end)


def colour_tolerance(max_dev):
    """The bound on |project - reference-host| for a Lab value or a colour distance: the project's documented bound to
    the float64 evaluation of the formula, 1e-4, plus the reference-host's own measured largest
    distance from float64, which the fixture stores.  Neither number comes from the code under test."""
    return 1e-4 + float(max_dev)
