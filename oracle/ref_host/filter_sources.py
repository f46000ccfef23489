"""Copies the reference's sources for the host builds, without the parts that do not compile there.

TEST INFRASTRUCTURE ONLY.  The device functions of image_renderer.cuh, compute_point_clouds.cuh and compute_costs.cuh
are plain C++ (one thread per triangle, pixel or point; word atomics; no shared memory, barriers or textures), so they
compile for the host behind shim/ref_shim.h.  The launchers below them use <<< >>> and thrust containers and do not:
each is cut out by name, from the start of its definition to its closing brace.  cuda_icp's host sources (the two
scenes, get_normal, the kd-tree, thrust__pcd2Ab, ICP_Point2Plane_cpu) are plain C++ as they stand; only icp.cpp's Eigen
parts are cut -- the three includes, the 6 x 6 solve with its two helpers, and the legacy loop that multiplies Eigen
matrices -- and driver_icp.cpp supplies the solve.  A name that is not found is an error -- a reference that moved its
code must not give a build that silently leaves something in or out.  Cut lines stay as empty lines, so that the line
numbers of what remains are the reference's.

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

ICP_DIR = "cuda_icp"
# file (relative to ICP_DIR) -> (includes to cut, functions to cut, explicit instantiations to cut: name -> how many)
ICP_SOURCES = {
    "include/cuda_icp/geometry.h": ((), (), {}),
    "include/cuda_icp/common.h": ((), (), {}),
    "include/cuda_icp/depth_scene.h": ((), (), {}),
    "include/cuda_icp/pcd_scene.h": ((), (), {}),
    "include/cuda_icp/icp.h": ((), (), {}),
    "scene/common.cpp": ((), (), {}),
    "scene/depth_scene/depth_scene.cpp": ((), (), {}),
    "scene/pcd_scene/pcd_scene.cpp": ((), (), {}),
    "icp.cpp": (("Eigen/Core", "Eigen/Cholesky", "Eigen/Geometry"),
                ("TransformVector6dToMatrix4d", "eigen_to_custom", "eigen_slover_666",
                 "ICP_Point2Plane_cpu_global_memory_version"),
                {"ICP_Point2Plane_cpu_global_memory_version": 2}),
}

# what may stand in front of a function's name where it is defined or declared: a return type, with its qualifiers
_TYPE = r"[\w:<>,\*&\s]+?"
_NOT_A_TYPE = ("return", "else", "new", "delete", "throw", "case", "goto")


class FilterError(RuntimeError):
    pass


def _strip_comment(line: str) -> str:
    i = line.find("//")
    return line if i < 0 else line[:i]


def _statements(lines, name, where):
    """The statements of the form `<type> name(`, each as (first line, last line, kind): "definition" when a `{`
    comes before any `;` (last line: its closing brace), else "declaration" (last line: its `;`).  Calls (`x = name(`,
    `return name(`) are not of that form."""
    pat = re.compile(r"\s*(" + _TYPE + r")\s+" + re.escape(name) + r"\s*\(")
    out = []
    for i, ln in enumerate(lines):
        m = pat.match(_strip_comment(ln))
        if not m or m.group(1).split()[0] in _NOT_A_TYPE:
            continue
        depth, opened, end, kind = 0, False, None, None
        for j in range(i, len(lines)):
            code = _strip_comment(lines[j])
            for ch in code:
                if ch == "{":
                    depth += 1
                    opened = True
                elif ch == "}":
                    depth -= 1
                elif ch == ";" and not opened:
                    end, kind = j, "declaration"
                    break
            if kind is None and opened and depth == 0:
                end, kind = j, "definition"
            if kind is not None:
                break
        if kind is None:
            raise FilterError(f"{where}: `{name}(` at line {i + 1} neither ends nor closes")
        out.append((i, end, kind))
    return out


def cut_function(text: str, name: str, where: str) -> str:
    """text without the definition of the free function `<type> name(...) {...}`, with the `template <...>` line
    above it when there is one (the line ends are kept)."""
    lines = text.split("\n")
    st = _statements(lines, name, where)
    defs = [s for s in st if s[2] == "definition"]
    if len(defs) != 1:
        what = "a declaration, not a definition" if st and not defs else f"found {len(defs)}"
        raise FilterError(f"{where}: expected one definition of `{name}(`: {what}")
    first, last, _ = defs[0]
    above = first - 1
    while above >= 0 and not lines[above].strip():
        above -= 1
    if above >= 0 and re.match(r"\s*template\s*<[^;{}]*>\s*$", _strip_comment(lines[above])):
        first = above
    for i in range(first, last + 1):
        lines[i] = ""
    return "\n".join(lines)


def cut_instantiations(text: str, name: str, count: int, where: str) -> str:
    """text without the `count` explicit instantiations `template <type> name(...);`."""
    lines = text.split("\n")
    inst = [s for s in _statements(lines, name, where)
            if s[2] == "declaration" and re.match(r"\s*template\s+[^<]", lines[s[0]])]
    if len(inst) != count:
        raise FilterError(f"{where}: expected {count} explicit instantiations of `{name}(`, found {len(inst)}")
    for first, last, _ in inst:
        for i in range(first, last + 1):
            lines[i] = ""
    return "\n".join(lines)


def cut_include(text: str, header: str, where: str) -> str:
    """text without the one line `#include <header>`."""
    lines = text.split("\n")
    hits = [i for i, ln in enumerate(lines) if re.match(r"\s*#\s*include\s*[<\"]" + re.escape(header) + r"[>\"]", ln)]
    if len(hits) != 1:
        raise FilterError(f"{where}: expected one `#include <{header}>`, found {len(hits)}")
    lines[hits[0]] = ""
    return "\n".join(lines)


def _read(src, reference_root):
    if not os.path.isfile(src):
        raise FilterError(f"{src}: not found (PCORE_REFERENCE_ROOT = {reference_root})")
    with open(src, encoding="utf-8", errors="replace") as f:
        return f.read()


def _write(dst, text):
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w", encoding="utf-8") as f:
        f.write(text)


def filter_sources(reference_root: str, out_dir: str) -> list:
    """Writes the filtered sources under out_dir/cuda_renderer/... and out_dir/cuda_icp/...; returns the files
    written."""
    inc = os.path.join(reference_root, INCLUDE)
    written = []
    for rel, cuts in SOURCES.items():
        src = os.path.join(inc, rel)
        text = _read(src, reference_root)
        for name in cuts:
            text = cut_function(text, name, src)
        if "<<<" in text:
            raise FilterError(f"{src}: a kernel launch is left after cutting {cuts}")
        dst = os.path.join(out_dir, "cuda_renderer", rel)
        _write(dst, text)
        written.append(dst)
    for rel, (includes, functions, instantiations) in ICP_SOURCES.items():
        src = os.path.join(reference_root, ICP_DIR, rel)
        text = _read(src, reference_root)
        lines_before = text.count("\n")
        for header in includes:
            text = cut_include(text, header, src)
        for name, count in instantiations.items():
            text = cut_instantiations(text, name, count, src)
        for name in functions:
            text = cut_function(text, name, src)
        if functions and "Eigen" in text:
            raise FilterError(f"{src}: the word Eigen is left after cutting {includes + functions}")
        if "<<<" in text:
            raise FilterError(f"{src}: a kernel launch is left")
        assert text.count("\n") == lines_before
        dst = os.path.join(out_dir, ICP_DIR, rel)
        _write(dst, text)
        written.append(dst)
    return written
