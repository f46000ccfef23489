"""Copies the reference's stage headers for the host build, without their host launchers.

TEST INFRASTRUCTURE ONLY.  The device functions of image_renderer.cuh, compute_point_clouds.cuh and compute_costs.cuh
are plain C++ (one thread per triangle, pixel or point; word atomics; no shared memory, barriers or textures), so they
compile for the host behind shim/ref_shim.h.  The launchers below them use <<< >>> and thrust containers and do not:
each is cut out by name, from the start of its definition to its closing brace.  A name that is not found is an error
-- a reference that moved its code must not give a build that silently leaves something in or out.

Everything is written under oracle/_ref/src/, which git ignores: the reference's text never enters the repository.
"""
from __future__ import annotations

import os
import re

INCLUDE = "cuda_renderer/include/cuda_renderer"
# header (relative to INCLUDE) -> the host functions to cut out of it
SOURCES = {
    "model.h": (),
    "cuda/utils.cuh": (),
    "cuda/image_renderer.cuh": ("image_render",),
    "cuda/compute_point_clouds.cuh": ("compute_point_clouds",),
    "cuda/compute_costs.cuh": ("compute_costs",),
}


class FilterError(RuntimeError):
    pass


def _strip_comment(line: str) -> str:
    i = line.find("//")
    return line if i < 0 else line[:i]


def cut_function(text: str, name: str, where: str) -> str:
    """text without the definition of the free function `void name(...) {...}` (with its line ends kept, so that
    the line numbers of what remains are the reference's)."""
    lines = text.split("\n")
    starts = [i for i, ln in enumerate(lines) if re.match(r"\s*void\s+" + re.escape(name) + r"\s*\(", ln)]
    if len(starts) != 1:
        raise FilterError(f"{where}: expected one definition of `void {name}(`, found {len(starts)}")
    depth, opened, end = 0, False, None
    for i in range(starts[0], len(lines)):
        code = _strip_comment(lines[i])
        if not opened and ";" in code and "{" not in code:
            raise FilterError(f"{where}: `void {name}(` is a declaration, not a definition")
        for ch in code:
            if ch == "{":
                depth += 1
                opened = True
            elif ch == "}":
                depth -= 1
        if opened and depth == 0:
            end = i
            break
    if end is None:
        raise FilterError(f"{where}: no closing brace for `void {name}(`")
    for i in range(starts[0], end + 1):
        lines[i] = ""
    return "\n".join(lines)


def filter_sources(reference_root: str, out_dir: str) -> list:
    """Writes the filtered headers under out_dir/cuda_renderer/...; returns the files written."""
    inc = os.path.join(reference_root, INCLUDE)
    written = []
    for rel, cuts in SOURCES.items():
        src = os.path.join(inc, rel)
        if not os.path.isfile(src):
            raise FilterError(f"{src}: not found (PCORE_REFERENCE_ROOT = {reference_root})")
        with open(src, encoding="utf-8", errors="replace") as f:
            text = f.read()
        for name in cuts:
            text = cut_function(text, name, src)
        if "<<<" in text:
            raise FilterError(f"{src}: a kernel launch is left after cutting {cuts}")
        dst = os.path.join(out_dir, "cuda_renderer", rel)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        with open(dst, "w", encoding="utf-8") as f:
            f.write(text)
        written.append(dst)
    return written
