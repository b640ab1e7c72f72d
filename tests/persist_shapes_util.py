"""tests/cpp/persist_shapes.cpp compiled with the host compiler and its output parsed: the row lists of csrc/persist_shapes.h and
persist_shape's answer over that program's domain.  Shared by the tests that hold the header against something else."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_and_parse(workdir):
    """(rows, shapes): rows[list] = [(B, mg, ebm, one, nptx), ...] for the lists main, k4, cases and variants;
    shapes[(B, nranks, grid, tiles_per_wg, eb_mode, members)] = ((B, mg, ebm, one, nptx), members) or None."""
    exe = os.path.join(str(workdir), "persist_shapes")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "magnetite_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "persist_shapes.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    rows = {"main": [], "k4": [], "cases": [], "variants": []}
    shapes = {}
    for ln in out:
        w = ln.split()
        if w[0] == "row":
            v = [int(x) for x in w[2:]]
            rows[w[1]].append((v[0], bool(v[1]), v[2], bool(v[3]), v[4]))
        else:
            assert w[0] == "shape" and w[7] == ":"
            key = tuple(int(x) for x in w[1:7])
            assert key not in shapes
            if w[8] == "none":
                shapes[key] = None
            else:
                v = [int(x) for x in w[8:]]
                shapes[key] = ((v[0], bool(v[1]), v[2], bool(v[3]), v[4]), v[5])
    return rows, shapes
