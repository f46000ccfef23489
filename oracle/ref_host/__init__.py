"""The reference's own stage kernels and ICP sources, compiled for the host -- TEST INFRASTRUCTURE ONLY (README.md in
this folder).

oracle.build_ref() builds oracle/_ref/ref_host, ref_icp and their _san twins from the reference root; this module writes
a request, runs one of the programs on it and reads the result.  The programs are stand-alone: nothing of them is
loaded into Python.  They exist only where the reference root does (the golden generator and the freshness test)."""
from __future__ import annotations

import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(os.path.dirname(_HERE), "_ref")
DEFAULT_ROOT = "/root/reference"

OP_RENDER, OP_CLOUD, OP_COSTS, OP_COLOUR = 1, 2, 3, 4                    # ref_host (driver.cpp)
OP_ICP_SCENE, OP_ICP_ROWS, OP_ICP_RUN, OP_ICP_DEPTH2CLOUD = 11, 12, 13, 14  # ref_icp (driver_icp.cpp)
_DTYPES = [np.dtype(np.uint8), np.dtype(np.int32), np.dtype(np.float32), np.dtype(np.float64)]


def reference_root() -> str:
    return os.environ.get("PCORE_REFERENCE_ROOT", DEFAULT_ROOT)


def have_reference() -> bool:
    return os.path.isdir(os.path.join(reference_root(), "cuda_renderer", "include", "cuda_renderer"))


class SanitizerReport(RuntimeError):
    pass


def write_bundle(path, arrays: dict):
    """name -> array (uint8 / int32 / float32 / float64, at most 4 dimensions; Python scalars become one int32 or
    float32); None values are left out."""
    items = []
    for name, a in arrays.items():
        if a is None:
            continue
        if isinstance(a, (bool, int, np.integer)):
            a = np.array([a], np.int32)
        elif isinstance(a, (float, np.floating)) and not isinstance(a, np.float64):
            a = np.array([a], np.float32)
        elif isinstance(a, np.float64):
            a = np.array([a], np.float64)
        a = np.ascontiguousarray(a)
        if a.dtype not in _DTYPES or a.ndim > 4 or len(name.encode()) > 23:
            raise ValueError(f"{name}: dtype {a.dtype}, ndim {a.ndim}")
        items.append((name, a))
    with open(path, "wb") as f:
        f.write(b"RHB1")
        f.write(np.int32(len(items)).tobytes())
        for name, a in items:
            f.write(name.encode().ljust(24, b"\0"))
            f.write(np.array([_DTYPES.index(a.dtype), a.ndim], np.int32).tobytes())
            f.write(np.array(list(a.shape) + [0] * (4 - a.ndim), np.int64).tobytes())
            raw = a.tobytes()
            f.write(raw)
            f.write(b"\0" * ((8 - len(raw) % 8) % 8))


def read_bundle(path) -> dict:
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:4] != b"RHB1":
        raise ValueError(f"{path}: not a result file")
    n = int(np.frombuffer(buf, np.int32, 1, 4)[0])
    off, out = 8, {}
    for _ in range(n):
        name = buf[off:off + 24].split(b"\0")[0].decode()
        dtype, ndim = (int(v) for v in np.frombuffer(buf, np.int32, 2, off + 24))
        shape = tuple(int(v) for v in np.frombuffer(buf, np.int64, 4, off + 32)[:ndim])
        off += 64
        cnt = int(np.prod(shape, dtype=np.int64)) if ndim else 1
        nbytes = cnt * _DTYPES[dtype].itemsize
        out[name] = np.frombuffer(buf, _DTYPES[dtype], cnt, off).reshape(shape).copy()
        off += (nbytes + 7) // 8 * 8
    return out


def run(request: dict, sanitized: bool = True, program: str = "ref_host") -> dict:
    """One request through <program>_san (or <program>): the result arrays.  Anything on the program's stderr, or a
    non-zero exit, is an error: with the sanitized build that is how an out-of-bounds access or undefined behaviour in
    the reference's code shows.  What it prints to stdout is dropped (get_normal and init_Scene_nn_cpu announce
    themselves there)."""
    exe = os.path.join(REF_DIR, program + ("_san" if sanitized else ""))
    if not os.path.exists(exe):
        raise FileNotFoundError(f"{exe}: run oracle.build_ref() first")
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0:halt_on_error=1"  # leaks cannot spoil a golden; LeakSanitizer needs ptrace
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    with tempfile.TemporaryDirectory(prefix="ref_host_") as tmp:
        req, res = os.path.join(tmp, "request.bin"), os.path.join(tmp, "result.bin")
        write_bundle(req, request)
        p = subprocess.run([exe, req, res], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
        if p.returncode != 0 or p.stderr.strip():
            raise SanitizerReport(f"{os.path.basename(exe)} op {request.get('op')}: exit {p.returncode}\n{p.stderr[-4000:]}")
        return read_bundle(res)
