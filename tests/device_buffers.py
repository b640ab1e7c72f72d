"""Caller-owned HBM for the tests of MAG_MEM_DEVICE, through ctypes on the HIP runtime the library itself loaded -- no torch in
the process (bench.py explains the import order) -- and the entry points of include/magnetite_hip.h that take a `memory`, wrapped
so that the host and the device leg of a test differ in that one argument.

DeviceArena hands out device buffers for numpy arrays.  Every buffer lies between two guard bands of GUARD bytes filled with a
fixed pattern; check() asserts that every band is intact and that every input still reads as it was uploaded (or scribbled), so
a copy of one byte too many or at a wrong offset fails there instead of corrupting a neighbour, and a library that wrote into its
caller's inputs is caught.  offset=8 places a payload on an 8-byte boundary that is no 16-byte boundary: the ABI promises the
alignment of double, no more.  Every HIP return code is asserted; close() (the `with` statement's finally) frees every buffer.

Leg(ctx, memory, arena) calls the entry points on one Context with arrays on the host or in the arena; arena.check() runs after
every call of the device leg."""
import ctypes as C

import numpy as np

from magnetite_amd import _lib
from magnetite_amd._lib import MAG_MEM_DEVICE, MAG_MEM_HOST, MAG_OK

GUARD = 256
GUARD_BYTE = 0xA5
H2D, D2H = 1, 2
# what an output holds before the call, another byte on either leg: a part the library left unwritten differs between the legs
UNWRITTEN = {MAG_MEM_HOST: 0x3C, MAG_MEM_DEVICE: 0xC3}
DP = C.POINTER(C.c_double)


def _hip():
    _lib.lib()  # pulls in the HIP runtime the library links
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipDeviceSynchronize.argtypes = []
    return hip


class DeviceBuffer:
    """A payload of `nbytes` at `ptr`, inside an allocation of the arena's; `expect`: the bytes an input must keep."""

    def __init__(self, base, lead, nbytes, dtype, shape, expect):
        self.base, self.lead, self.nbytes, self.dtype, self.shape, self.expect = base, lead, nbytes, dtype, shape, expect
        self.ptr = base + lead
        self.total = lead + nbytes + GUARD


class HostBuffer:
    """The host leg's twin of a DeviceBuffer: a numpy array of the test's own, between guard bands as well (a copy of one byte
    too many into host memory is then an assertion of check(), not a corrupted heap)."""

    def __init__(self, array):
        flat = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        self.image = np.full(GUARD + flat.size + GUARD, GUARD_BYTE, dtype=np.uint8)
        self.image[GUARD:GUARD + flat.size] = flat
        self.array = self.image[GUARD:GUARD + flat.size].view(array.dtype).reshape(array.shape)
        self.ptr = self.array.ctypes.data

    def check(self):
        n = self.image.size - GUARD
        assert (self.image[:GUARD] == GUARD_BYTE).all() and (self.image[n:] == GUARD_BYTE).all(), ("guard band of a host buffer", self.array.shape)


class DeviceArena:
    def __init__(self):
        self.hip = _hip()
        self.buffers = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        try:
            for b in self.buffers:
                assert self.hip.hipFree(C.c_void_p(b.base)) == 0
        finally:
            self.buffers = []

    def _allocate(self, payload, dtype, shape, offset, is_input):
        assert offset % np.dtype(dtype).itemsize == 0 and 0 <= offset < GUARD
        lead = GUARD + offset
        image = np.full(lead + payload.size + GUARD, GUARD_BYTE, dtype=np.uint8)
        image[lead:lead + payload.size] = payload
        base = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(base), image.size) == 0
        b = DeviceBuffer(base.value, lead, payload.size, np.dtype(dtype), shape, payload.copy() if is_input else None)
        self.buffers.append(b)  # (listed before the copy: close() frees it whatever happens next)
        assert b.base % 256 == 0  # hipMalloc's alignment: the payload's is then lead's
        assert self.hip.hipMemcpy(C.c_void_p(b.base), image.ctypes.data, image.size, H2D) == 0
        return b

    def put(self, array, offset=0):
        """An input: the array's bytes on the device.  check() asserts they stay."""
        a = np.ascontiguousarray(array)
        return self._allocate(a.reshape(-1).view(np.uint8), a.dtype, a.shape, offset, True)

    def empty(self, shape, dtype=np.float64, offset=0):
        """An output, every byte UNWRITTEN."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self._allocate(np.full(n, UNWRITTEN[MAG_MEM_DEVICE], dtype=np.uint8), dtype, tuple(np.atleast_1d(shape)), offset, False)

    def _image(self, b):
        image = np.empty(b.total, dtype=np.uint8)
        assert self.hip.hipMemcpy(image.ctypes.data, C.c_void_p(b.base), b.total, D2H) == 0
        return image

    def read(self, b):
        return self._image(b)[b.lead:b.lead + b.nbytes].view(b.dtype).reshape(b.shape).copy()

    def scribble(self, b):
        """0xFF over the payload: every double a NaN.  What a caller may do with its buffer once a call has returned."""
        ff = np.full(b.nbytes, 0xFF, dtype=np.uint8)
        assert self.hip.hipMemcpy(C.c_void_p(b.ptr), ff.ctypes.data, b.nbytes, H2D) == 0
        if b.expect is not None:
            b.expect = ff

    def free(self, *buffers):
        for b in buffers:
            self.buffers.remove(b)
            assert self.hip.hipFree(C.c_void_p(b.base)) == 0

    def check(self):
        """Every guard band intact, every input as it was uploaded (or scribbled)."""
        assert self.hip.hipDeviceSynchronize() == 0
        for k, b in enumerate(self.buffers):
            image = self._image(b)
            before, after = image[:b.lead], image[b.lead + b.nbytes:]
            assert (before == GUARD_BYTE).all(), ("guard band before buffer", k, b.shape, np.flatnonzero(before != GUARD_BYTE)[:8] - b.lead)
            assert (after == GUARD_BYTE).all(), ("guard band after buffer", k, b.shape, np.flatnonzero(after != GUARD_BYTE)[:8])
            if b.expect is not None:
                now = image[b.lead:b.lead + b.nbytes]
                assert np.array_equal(now, b.expect), ("the library wrote into an input", k, b.shape, np.flatnonzero(now != b.expect)[:8])


def _dp(ptr):
    return None if ptr is None else C.cast(C.c_void_p(ptr), DP)


class Leg:
    """The entry points that take a `memory`, on one Context, with every array in `memory`: numpy arrays of the leg's own
    (MAG_MEM_HOST) or buffers of `arena` (MAG_MEM_DEVICE, payloads at `offset`).  Calls that take inputs return the status
    (error() gives the message); `scribble` overwrites the inputs with 0xFF once the call has returned.  Downloads assert MAG_OK
    and return numpy arrays, None for a member passed as NULL."""

    def __init__(self, ctx, memory, arena=None, offset=0):
        assert memory == MAG_MEM_HOST or arena is not None
        self.ctx, self.memory, self.arena, self.offset = ctx, memory, arena, offset
        self.L, self.h = ctx._L, ctx._h
        self.device = memory == MAG_MEM_DEVICE

    # -- buffers of the leg's memory
    def _in(self, a, dtype=np.float64):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        return self.arena.put(a, self.offset) if self.device else HostBuffer(a)

    def _out(self, shape, dtype=np.float64, offset=None):
        if shape is None:
            return None
        if self.device:
            return self.arena.empty(shape, dtype, self.offset if offset is None else offset)
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return HostBuffer(np.full(n, UNWRITTEN[MAG_MEM_HOST], dtype=np.uint8).view(dtype).reshape(shape))

    def _get(self, b):
        if b is None:
            return None
        return self.arena.read(b) if self.device else b.array.copy()

    @staticmethod
    def _ptr(b):
        return None if b is None else b.ptr

    def _called(self, inputs=(), outputs=(), scribble=False, keep=False):
        """After every call: the bands and the inputs; then the inputs may be scribbled over (and are checked again, as 0xFF, by
        every later check when kept) and the call's buffers go."""
        inputs, outputs = [b for b in inputs if b is not None], [b for b in outputs if b is not None]
        if self.device:
            self.arena.check()
        else:
            for b in inputs + outputs:
                b.check()
        for b in inputs:
            if scribble and self.device:
                self.arena.scribble(b)
            elif scribble:
                b.array.reshape(-1).view(np.uint8)[:] = 0xFF
        got = [self._get(b) for b in outputs]
        if self.device:
            self.arena.free(*([] if keep else inputs), *outputs)
        return got

    def error(self):
        return self.L.mag_last_error(self.h).decode()

    def _ok(self, rc):
        assert rc == MAG_OK, (rc, self.error())

    # -- mag_solve: problem and result in `memory`
    def solve(self, prob):
        N, E = prob.mesh.num_nodes, prob.mesh.num_elements
        ins = [self._in(a, t) for a, t in ((prob.xy_flat, np.float64), (prob.conn_flat, np.int32), (prob.u_known, np.uint8),
                                           (prob.u_in, np.float64), (prob.f_in, np.float64))]
        outs = [self._out(n) for n in (2 * N, 2 * N, E)]
        p = _lib.Problem(N, E, *[b.ptr for b in ins], prob.youngs_modulus, prob.poisson_ratio, prob.part_thickness, self.memory, 0)
        r = _lib.Result(*[b.ptr for b in outs], self.memory, 0)
        self._ok(self.L.mag_solve(self.h, C.byref(p), C.byref(r)))
        self.ctx.N, self.ctx.E = N, E
        return self._called(ins, outs, scribble=True)

    # -- load cases and variants
    def set_load_cases(self, u_in, f_in, scribble=True):
        ins = [self._in(u_in), self._in(f_in)]
        rc = self.L.mag_set_load_cases(self.h, len(u_in), _dp(ins[0].ptr), _dp(ins[1].ptr), self.memory)
        self._called(ins, scribble=scribble, keep=True)
        return rc

    def set_variants(self, V, xy=None, material=None, u_in=None, f_in=None, scribble=True):
        ins = [self._in(a) for a in (xy, material, u_in, f_in)]
        rc = self.L.mag_set_variants(self.h, V, *[_dp(self._ptr(b)) for b in ins], self.memory)
        self._called(ins, scribble=scribble, keep=True)
        return rc

    def _download_member(self, fn, i):
        outs = [self._out(n) for n in (2 * self.ctx.N, 2 * self.ctx.N, self.ctx.E)]
        r = _lib.Result(*[b.ptr for b in outs], self.memory, 0)
        self._ok(fn(self.h, i, C.byref(r)))
        return dict(zip(("u", "f", "stress"), self._called(outputs=outs)))

    def download_case(self, i):
        return self._download_member(self.L.mag_download_case, i)

    def download_variant(self, i):
        return self._download_member(self.L.mag_download_variant, i)

    # -- the four derived passes: `want` names the members asked for, the others are passed as NULL
    def _download_rows(self, fn, struct, rows, set, i, want):
        want = tuple(rows) if want is None else want
        outs = [self._out(shape if name in want else None) for name, shape in rows.items()]
        o = struct(*[self._ptr(b) for b in outs], (C.c_double * 8)(*([np.nan] * 8)), self.memory, 0)
        self._ok(fn(self.h, self.ctx.SENSITIVITY_SETS[set], i, C.byref(o)))
        got = self._called(outputs=outs)  # (the NULL members are dropped by _called: `got` holds the wanted ones in order)
        out = dict(zip([name for name in rows if name in want], got))
        out["scalars"] = np.array(list(o.scalars))
        return out

    def download_sensitivity(self, set, i, want=None):
        N, E = self.ctx.N, self.ctx.E
        return self._download_rows(self.L.mag_download_sensitivity, _lib.Sensitivity, dict(energy=E, dxy=2 * N), set, i, want)

    def download_adjoint(self, set, i, want=None):
        N, E = self.ctx.N, self.ctx.E
        rows = {"lambda": 2 * N, "dloads": 2 * N, "delem": E, "dxy": 2 * N}
        return self._download_rows(self.L.mag_download_adjoint, _lib.Adjoint, rows, set, i, want)

    def download_objective(self, set, i, want=("g", "pxy")):
        N = self.ctx.N
        return self._download_rows(self.L.mag_download_objective, _lib.ObjectiveResult, dict(g=2 * N, pxy=2 * N, dxy=2 * N), set, i, want)

    def download_stress(self, set, i, want=None):
        N, E = self.ctx.N, self.ctx.E
        return self._download_rows(self.L.mag_download_stress, _lib.StressField, dict(elem=(E, 4), node=(N, 4), eta2=E), set, i, want)

    def run_adjoint(self, set, dJ_du, scribble=True):
        g = self._in(dJ_du)
        rc = self.L.mag_run_adjoint(self.h, self.ctx.SENSITIVITY_SETS[set], _dp(g.ptr), self.memory)
        self._called([g], scribble=scribble)
        return rc

    def run_objective(self, set, kind, weights=None, target=None, per_member=0, p=8.0, scale=1.0, with_adjoint=0):
        """The rows are read where they are: they are the caller's until the call returns, and unchanged then (_called)."""
        w, t = self._in(weights), self._in(target)
        o = _lib.Objective(self.ctx.OBJECTIVE_KINDS[kind], per_member, float(p), float(scale), self._ptr(w), self._ptr(t), self.memory, 0)
        rc = self.L.mag_run_objective(self.h, self.ctx.SENSITIVITY_SETS[set], C.byref(o), with_adjoint)
        self._called([w, t], scribble=True)
        return rc

    # -- refinement
    def run_refine(self, rule, split=1, theta=0.5, marks=None, indicator=None):
        m, ind = self._in(marks, np.uint8), self._in(indicator)
        o = _lib.RefineOptions(self.ctx.REFINE_RULES[rule], split, float(theta), self._ptr(m), self._ptr(ind), self.memory, 0)
        rc = self.L.mag_run_refine(self.h, C.byref(o))
        self._called([m, ind], scribble=True)
        return rc

    REFINED = (("xy", np.float64), ("conn", np.int32), ("u_known", np.uint8), ("u_in", np.float64), ("f_in", np.float64),
               ("node_parents", np.int32), ("elem_parent", np.int32))

    def download_refine(self):
        """Every array of the refined mesh; node_parents always gets a buffer (two words at least): where no node was added it
        comes back UNWRITTEN."""
        info = self.ctx.refine_info()
        Nn, En, added = info["nodes"], info["elements"], info["marked_edges"]
        shapes = dict(xy=(Nn, 2), conn=(En, 3), u_known=(2 * Nn,), u_in=(2 * Nn,), f_in=(2 * Nn,), node_parents=(max(added, 1), 2), elem_parent=(En,))
        outs = [self._out(shapes[name], dtype) for name, dtype in self.REFINED]
        self._ok(self.L.mag_download_refine(self.h, C.byref(_lib.Refined(*[b.ptr for b in outs], self.memory, 0))))
        out = dict(zip([name for name, _ in self.REFINED], self._called(outputs=outs)))
        out.update(info)
        return out

    # -- modal analysis
    def download_modal(self):
        p = self.ctx.modal_info()["modes"]
        outs = [self._out(p), self._out(p), self._out(p), self._out((p, 2 * self.ctx.N))]
        self._ok(self.L.mag_download_modal(self.h, C.byref(_lib.ModalResult(*[b.ptr for b in outs], self.memory, 0))))
        return dict(zip(("lambda", "frequency", "residual", "shapes"), self._called(outputs=outs)))

    # -- transient dynamics
    TRANSIENT = (("u", "u_out"), ("v", "v_out"), ("a", "a_out"), ("f", "f_out"), ("probe_u", "probe_u"), ("probe_v", "probe_v"),
                 ("probe_a", "probe_a"), ("energies", "energies"), ("snapshots", "snapshots"), ("iterations", "iterations"))

    def run_transient(self, steps, dt, density, amplitude=None, u0=None, v0=None, probes=None, scribble=True, **options):
        """amplitude, u0, v0 and the int32 probes in `memory` (the probes on a 4-byte boundary that is no 8-byte one where the
        doubles lie at an offset); `options`: the other fields of mag_transient_options by name.  The inputs stay allocated,
        scribbled over: a resumed run that read them again would step with NaNs, and every later check() sees them as 0xFF."""
        ins = [self._in(amplitude), self._in(u0), self._in(v0)]
        p = None
        if probes is not None:
            p = np.ascontiguousarray(probes, dtype=np.int32)
            p = self.arena.put(p, 4 if self.offset else 0) if self.device else HostBuffer(p)
        o = _lib.TransientOptions()
        self.L.mag_default_transient_options(C.byref(o))
        o.steps, o.dt, o.density, o.memory = int(steps), float(dt), float(density), self.memory
        o.amplitude, o.u0, o.v0, o.probes = (self._ptr(b) for b in ins + [p])
        o.num_probes = 0 if probes is None else len(probes)
        for k, v in options.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
        rc = self.L.mag_run_transient(self.h, C.byref(o))
        self._called(ins + [p], scribble=scribble, keep=True)
        self._transient = (o.num_probes, bool(o.energies))  # (what download_transient sizes)
        return rc

    def download_transient(self, want=None, slack=3):
        """Every array of the result struct (`want` names the members asked for, the others are passed as NULL), iterations as
        int32, t_start and t_end.  Every buffer has room for `slack` entries more than the header documents: they must come
        back UNWRITTEN."""
        info = self.ctx.transient_info()
        rows, n2, (num_probes, energies) = info["steps"] + 1, 2 * self.ctx.N, self._transient
        shapes = dict(u=(n2,), v=(n2,), a=(n2,), f=(n2,), probe_u=(rows, num_probes), probe_v=(rows, num_probes), probe_a=(rows, num_probes),
                      energies=(rows, 3), snapshots=(info["snapshots_kept"], n2), iterations=(rows,))
        want = tuple(k for k, _ in self.TRANSIENT if int(np.prod(shapes[k])) > 0 and (energies or k != "energies")) if want is None else want
        outs = {k: self._out(int(np.prod(shapes[k])) + slack if k in want else None) for k, _ in self.TRANSIENT if k != "iterations"}
        # (the int32 buffer on a 4-byte boundary, like the probes)
        outs["iterations"] = self._out(rows + slack if "iterations" in want else None, np.int32, 4 if self.offset else 0)
        o = _lib.TransientResult(memory=self.memory, scalars=(C.c_double * 4)(*([np.nan] * 4)))
        for k, member in self.TRANSIENT:
            setattr(o, member, self._ptr(outs[k]))
        self._ok(self.L.mag_download_transient(self.h, C.byref(o)))
        got = self._called(outputs=list(outs.values()))
        out = {}
        for k, flat in zip([k for k, _ in self.TRANSIENT if k in want], got):
            n = int(np.prod(shapes[k]))
            assert (flat[n:].view(np.uint8) == UNWRITTEN[self.memory]).all(), ("written beyond its documented size", k)
            out[k] = flat[:n].reshape(shapes[k])
        out["t_start"], out["t_end"] = float(o.scalars[0]), float(o.scalars[1])
        return out

    def assemble_effective(self, c_K, c_M, density, lumped=False, slack=3):
        """c_K K + c_M M in the layout of assemble_csr(), into `memory`; `slack` entries behind it stay UNWRITTEN"""
        n = self.ctx.assemble_csr()[2].size
        out = self._out(n + slack)
        self._ok(self.L.mag_assemble_effective(self.h, float(c_K), float(c_M), float(density), 1 if lumped else 0, _dp(out.ptr), self.memory))
        flat, = self._called(outputs=[out])
        assert (flat[n:].view(np.uint8) == UNWRITTEN[self.memory]).all(), "written beyond its documented size"
        return flat[:n]

    # -- the element stiffness field and the design
    def set_element_scale(self, scale):
        s = self._in(scale)
        rc = self.L.mag_set_element_scale(self.h, _dp(s.ptr), self.memory)
        self._called([s], scribble=True)
        return rc

    def design_init(self, rho0, **options):
        o = _lib.DesignOptions(**{**dict(volume_fraction=0.5, scale_min=1e-3, rho_min=1e-3, move=0.2, penal=3, filter_passes=1), **options})
        r = self._in(rho0)
        rc = self.L.mag_design_init(self.h, C.byref(o), _dp(r.ptr), self.memory)
        self._called([r], scribble=True)
        return rc

    def design_step(self, dJ_ds):
        g = self._in(dJ_ds)
        rc = self.L.mag_design_step(self.h, _dp(g.ptr), self.memory)
        self._called([g], scribble=True)
        return rc

    def download_design(self):
        outs = [self._out(self.ctx.E) for _ in range(4)]
        self._ok(self.L.mag_download_design(self.h, C.byref(_lib.Design(*[b.ptr for b in outs], self.memory, 0))))
        return dict(zip(("rho", "rho_filtered", "scale", "dJ_drho"), self._called(outputs=outs)))
