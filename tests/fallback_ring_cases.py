"""Cases for the certified fragment depth's IEEE fallback in the depth pass of fastdiv and interior poses
(raster_phase, pcore_fused.hip): there the vertex ring holds v_rcp_f32(z) instead of z, and a lane that takes the
fallback computes its three depths again from the vertex stream -- the latest pass written into the slot's ring buffer.

Every model is made of fronto-parallel right triangles ("patches") at camera depths k + 0.5 cm, k = 40 ... 199, each
placed at random inside the part of the image that the model's box shows at its depth: the box is a cuboid whose near
face fills the image's middle 140 x 104 pixels, so a patch at depth d lies within 40.5 / d of that around the
principal point, and patches of different depths overlap on the screen.  The fragment depth int(Q + 0.5) of such a
patch has Q within a few 2^-24 Q of the half-integer, inside the certificate's bracket, so every covered sample takes
the fallback (tests/test_fallback_ring_cases.py certifies it on a float32 restatement).  Three models, each a bank of its own,
uploaded with the number of streams its walk needs (PCORE_MODEL_STREAMS, read by upload_meshes):
  wrap   150 patches in ONE stream: 8 vertex passes, the ring of 4 wraps
  switch 456 patches in 8 streams: each wave walks two streams and flushes the first one's records after loading
         the second one's header
  one    one triangle
and two poses each: `interior` (class 2, the image's middle) and `border` (class 1, shifted across the left border).
tests/test_gpu_depth_fallback_ring.py runs them bit for bit against the oracle."""
from __future__ import annotations

import functools

import numpy as np

from tests import interior_cases as ic
from tests import mesh_cases as mc

F32 = np.float32
CAM = mc.CAM               # 160 x 120
STRIDES = (8, 2)           # the templated kernel and a generic stride at which every patch covers samples
MODELS = {"wrap": (150, 1), "switch": (456, 8), "one": (1, None)}  # patches, PCORE_MODEL_STREAMS
K_LO, K_HI = 40, 199
T_Z = 0.405                # metres: the poses' depth translation; a patch at depth k + 0.5 cm has model z (k - 40) cm
CENTRE = (CAM["cx"], CAM["height"] - CAM["cy"])  # the principal point in screen coordinates
HALF = (70.0, 52.0)        # pixels: half the near face of the model's box on the screen (interior pose)
SIZE = 5.2                 # pixels: a patch's legs
SHIFT = -12.0              # pixels: the border pose's shift of the 40.5 cm layer (nearer layers move more)


def _model_z(k):
    """Model z (metres, float32) of depth k + 0.5 cm: 100 * z + 40.5 is k + 0.5 exactly in float32."""
    z0 = F32((k - K_LO) / 100.0)
    for z in (z0, np.nextafter(z0, F32(1)), np.nextafter(z0, F32(-1))):
        if F32(100) * z + F32(40.5) == F32(k + 0.5):
            return z
    raise AssertionError(k)


def _unproject(u, v, depth_cm):
    """Model (x, y) in metres that the interior pose shows at screen (u, v) at camera depth depth_cm."""
    W, H = CAM["width"], CAM["height"]
    p = ic.proj(CAM).astype(np.float64)
    x = ((u - W / 2) / (W / 2) - p[2]) * depth_cm / p[0]
    y = ((v - H / 2) / (H / 2) - p[6]) * depth_cm / p[5]
    return x / 100.0, y / 100.0


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(T, 9) float32 and the k of every triangle."""
    n, _ = MODELS[name]
    rng = np.random.default_rng(41 + n)
    tris, ks = [], []
    for c in range(n):
        if name == "one":
            k, size, u0, v0 = 57, 34.0, 8.0, 30.0
        else:
            k, size = K_LO + (c * 37) % (K_HI - K_LO + 1), SIZE
            sc = 40.5 / (k + 0.5)
            u0 = CENTRE[0] - HALF[0] * sc + rng.random() * (2 * HALF[0] * sc - size)
            v0 = CENTRE[1] - HALF[1] * sc + rng.random() * (2 * HALF[1] * sc - size)
        z = _model_z(k)
        corner = int(rng.integers(4))
        q = np.array([(u0, v0), (u0 + size, v0), (u0 + size, v0 + size), (u0, v0 + size)])
        q = np.delete(q, corner, axis=0)
        x, y = _unproject(q[:, 0], q[:, 1], k + 0.5)
        tris.append(np.c_[x, y, np.full(3, z)].reshape(9))
        ks.append(k)
    return mc._frozen(np.asarray(tris, F32)), np.asarray(ks)


def _rows(t_cm):
    m = np.zeros(16, F32)
    m[:12] = np.c_[np.eye(3) * 100.0, np.asarray(t_cm, np.float64)].astype(F32).reshape(-1)
    m[15] = 1
    return m


POSE_KINDS = ("interior", "border")
# the border pose moves the model by SHIFT pixels of the 40.5 cm layer: SHIFT * 40.5 / fx cm
POSES = np.stack([_rows((0.0, 0.0, T_Z * 100)), _rows((SHIFT * 40.5 / CAM["fx"], 0.0, T_Z * 100))])
POSES.setflags(write=False)


class FallbackCase(mc.MeshCase):
    """mesh_cases.MeshCase over one model of this module and its two poses."""

    def __init__(self, name):
        self.name = name
        self.tris_k = mesh(name)[1]
        self.bank = mc.Bank("fallback_" + name, [(name, mesh(name)[0], None)])
        self.streams = MODELS[name][1]
        self.cam = CAM
        self.width, self.height = CAM["width"], CAM["height"]
        self.proj = ic.proj(CAM)
        self.poses = POSES
        self.poses44 = None
        self.n = len(POSES)
        self.pose_model = np.zeros(self.n, np.int32)
        self.pose_label = self.pose_model.copy()
        self.pose_kind = np.arange(self.n)
        self.src_depth = np.zeros((self.height, self.width), np.int32)
        self.mask = np.zeros((self.height, self.width), np.uint8)
        self.r = mc.R
        self.oracle_count = np.concatenate([self.bank.tris_model_count, [0]]).astype(np.int32)

    def describe(self, pose):
        return f"model {self.name}, pose {pose} ({POSE_KINDS[pose]})"

    def fragments(self, pose, stride):
        """Every (triangle, sample) pair the raster tests with its fragment inside, from a float32 restatement of the
        vertex pass, the reference's bounding box and barycentrics, and the IEEE depth chain:
        (kx, ky, k of the triangle, Q) arrays."""
        f = F32
        s, W, H = stride, self.width, self.height
        v = self.bank.tris.reshape(-1, 3)
        sx, sy, lz = ic.vertex_pass(self.poses[pose], v, CAM)
        sx, sy, lz = sx.reshape(-1, 3), sy.reshape(-1, 3), lz.reshape(-1, 3)
        out = []
        for t in range(len(sx)):
            lo0, hi0 = max(f(0), sx[t].min()), min(f(W - 1), sx[t].max())
            lo1, hi1 = max(f(0), sy[t].min()), min(f(H - 1), sy[t].max())
            if hi0 < 0 or hi1 < 0:
                continue
            p0 = np.arange(int(lo0 + f(0.5)), int(np.floor(hi0)) + 1)
            p1 = np.arange(int(lo1 + f(0.5)), int(np.floor(hi1)) + 1)
            p0 = p0[p0 % s == 0]
            p1 = p1[(H - 1 - p1) % s == 0]
            if not len(p0) or not len(p1):
                continue
            P0, P1 = (a.ravel().astype(F32) for a in np.meshgrid(p0, p1))
            (A0, B0, C0), (A1, B1, C1) = sx[t], sy[t]
            area = f(0.5) * ((C0 - A0) * (B1 - A1) - (B0 - A0) * (C1 - A1))
            with np.errstate(all="ignore"):
                inv = f(1) / area
                beta = f(0.5) * ((C0 - A0) * (P1 - A1) - (P0 - A0) * (C1 - A1)) * inv
                gamma = f(0.5) * ((P0 - A0) * (B1 - A1) - (B0 - A0) * (P1 - A1)) * inv
                alpha = f(1) - beta - gamma
                inside = ~((alpha < 0) | (beta < 0) | (gamma < 0) | (alpha > 1) | (beta > 1) | (gamma > 1))
                Q = (alpha + beta + gamma) / (alpha / lz[t, 0] + beta / lz[t, 1] + gamma / lz[t, 2])
            for a, b, q in zip(P0[inside], P1[inside], Q[inside]):
                out.append((int(a) // s, (H - 1 - int(b)) // s, int(self.tris_k[t]), float(q)))
        return np.array(out, np.float64).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def case(name):
    return FallbackCase(name)
