"""CPU: the C ABI of the nonlinear transient pass -- the sizes and offsets of mag_transient_tl_options (128 bytes) and
mag_transient_tl_result (40 bytes) as the C compiler lays them out against the ctypes binding, mag_transient_options untouched at
120 bytes, the new symbols exported, the defaults.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

from magnetite_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mag_default_transient_tl_options", "mag_run_transient_tl", "mag_download_transient_tl", "mag_get_transient_tl_info",
       "mag_assemble_effective_tangent")


def test_struct_layouts_match_header(built, tmp_path):
    structs = {"mag_transient_tl_options": _lib.TransientTlOptions, "mag_transient_tl_result": _lib.TransientTlResult,
               "mag_transient_options": _lib.TransientOptions}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "magnetite_hip.h"', "int main(void){"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
    assert int(got["mag_transient_tl_options"]) == 128 and int(got["mag_transient_tl_result"]) == 40
    assert int(got["mag_transient_options"]) == 120  # (pinned: the new pass has a struct of its own)
    assert int(got["mag_transient_tl_options.dt"]) == 40 and int(got["mag_transient_tl_options.amplitude"]) == 96
    assert int(got["mag_transient_tl_options.probes"]) == 120 and int(got["mag_transient_tl_result.memory"]) == 32
    assert not any(f == "rayleigh_stiffness" for f, _ in _lib.TransientTlOptions._fields_)


def test_the_new_symbols_are_exported(built):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH], text=True)
    exported = set(re.findall(r" T (mag_[a-z_0-9]+)", out))
    assert set(NEW) <= exported, set(NEW) - exported
    assert set(NEW) <= set(_lib.SYMBOLS)
    L = _lib.lib()
    for n in NEW:
        getattr(L, n)


def test_the_defaults(built):
    L = _lib.lib()
    o = _lib.TransientTlOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    L.mag_default_transient_tl_options(C.byref(o))
    assert (o.beta, o.gamma) == (0.25, 0.5)
    zero = [f for f, _ in _lib.TransientTlOptions._fields_ if f not in ("beta", "gamma")]
    assert all(not getattr(o, f) for f in zero), [f for f in zero if getattr(o, f)]
    L.mag_default_transient_tl_options(None)  # (a null pointer is ignored)
