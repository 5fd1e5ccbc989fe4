"""ctypes binding of the C-ABI in include/nimble_amd.h (libnimble_amd.so).

The product path has no CPU fallback: if the HIP library is missing or no
ROCm device is present, calls raise instead of silently computing elsewhere.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NIMBLE_AMD_LIB") or os.path.join(_HERE, "libnimble_amd.so")

_lib = None


# wrench_frame of the `_ext` entry points (include/nimble_amd.h)
WRENCH_WORLD, WRENCH_BODY = 0, 1
WRENCH_FRAMES = {"world": WRENCH_WORLD, "body": WRENCH_BODY}


def wrench_frame_flag(frame) -> int:
    """"world" / "body" (or the header's 0 / 1) -> NIMBLE_WRENCH_*."""
    if isinstance(frame, str):
        if frame not in WRENCH_FRAMES:
            raise ValueError(f"wrench_frame {frame!r}: expected 'world' or 'body'")
        return WRENCH_FRAMES[frame]
    if isinstance(frame, bool) or not isinstance(frame, int) or frame not in (WRENCH_WORLD, WRENCH_BODY):
        raise ValueError(f"wrench_frame {frame!r}: expected 'world' or 'body'")
    return int(frame)


def _ext_prototypes():
    """argtypes of the six entry points with external body wrenches: the
    `_pw` sibling's buffers (body_inertia the last of them), then body_wrench,
    wrench_frame, the wrench-gradient output where there is one, the stream."""
    v, i = C.c_void_p, C.c_int32
    head = [v, i]
    return {
        "nimble_forward_ext": head + [v] * 6 + [v, i, v],
        "nimble_backward_ext": head + [v] * 7 + [v, i, v, v],
        "nimble_backward_masses_ext": head + [v] * 8 + [v, i, v],
        "nimble_backward_inertia_ext": head + [v] * 8 + [v, i, v],
        "nimble_jacobians_ext": head + [v] * 7 + [v, i, v, v],
        "nimble_constraint_force_jacobians_ext": head + [v] * 7 + [v, i, v],
    }


EXT_PROTOTYPES = _ext_prototypes()


def _inverse_dynamics_prototypes():
    """argtypes of the two inverse-dynamics entry points (include/nimble_amd.h):
    world, batch, state, ddq, body_inertia, body_wrench, wrench_frame, then
    the outputs (forward: tau, mass_matrix, bias; backward: grad_tau in,
    grad_state, grad_ddq, grad_wrench out), the stream."""
    v, i = C.c_void_p, C.c_int32
    head = [v, i, v, v, v, v, i]
    return {
        "nimble_inverse_dynamics": head + [v, v, v] + [v],
        "nimble_inverse_dynamics_backward": head + [v, v, v, v] + [v],
    }


ID_PROTOTYPES = _inverse_dynamics_prototypes()


def _inverse_dynamics_inertia_prototypes():
    """argtypes of the two entry points for the inertial parameters of the
    inverse dynamics (include/nimble_amd.h): the backward's arguments with
    grad_inertia ahead of the stream; world, batch, state, ddq, body_inertia,
    jacobian, stream."""
    v, i = C.c_void_p, C.c_int32
    return {
        "nimble_invdyn_backward_inertia": [v, i, v, v, v, v, i] + [v, v, v, v, v] + [v],
        "nimble_invdyn_inertia_jacobian": [v, i, v, v, v, v] + [v],
    }


ID_INERTIA_PROTOTYPES = _inverse_dynamics_inertia_prototypes()


def _contact_inverse_dynamics_prototypes():
    """argtypes of nimble_contact_inverse_dynamics (include/nimble_amd.h): the
    head of the inverse-dynamics entry points, then num_contact_bodies,
    contact_bodies (host), wrench_guesses, tau, contact_wrenches, the stream."""
    v, i = C.c_void_p, C.c_int32
    return {"nimble_contact_inverse_dynamics": [v, i, v, v, v, v, i] + [i, v, v, v, v] + [v]}


CID_PROTOTYPES = _contact_inverse_dynamics_prototypes()
MAX_CONTACT_BODIES = 8  # NIMBLE_MAX_CONTACT_BODIES


class NativeLibraryMissing(ImportError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        L.nimble_world_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.nimble_world_create.restype = C.c_int
        L.nimble_world_destroy.argtypes = [C.c_void_p]
        L.nimble_world_destroy.restype = C.c_int
        L.nimble_snapshot_doubles.argtypes = [C.c_void_p]
        L.nimble_snapshot_doubles.restype = C.c_int64
        L.nimble_lcp_cache_doubles.argtypes = [C.c_void_p]
        L.nimble_lcp_cache_doubles.restype = C.c_int64
        L.nimble_forward.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_void_p]
        L.nimble_forward.restype = C.c_int
        L.nimble_backward.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_void_p]
        L.nimble_backward.restype = C.c_int
        L.nimble_backward_masses.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.c_void_p]
        L.nimble_backward_masses.restype = C.c_int
        L.nimble_backward_inertia.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.c_void_p]
        L.nimble_backward_inertia.restype = C.c_int
        L.nimble_last_error.argtypes = []
        L.nimble_last_error.restype = C.c_char_p
        L.nimble_jacobian_workspace_doubles.argtypes = [C.c_void_p, C.c_int32]
        L.nimble_jacobian_workspace_doubles.restype = C.c_int64
        L.nimble_jacobians.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_void_p]
        L.nimble_constraint_force_jacobians.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_void_p]
        L.nimble_constraint_force_jacobians.restype = C.c_int
        L.nimble_jacobians.restype = C.c_int
        L.nimble_num_collision_pairs.argtypes = [C.c_void_p]
        # the siblings with per-world body inertial parameters: body_inertia
        # ahead of the stream
        for name, buffers in (("nimble_forward_pw", 6), ("nimble_backward_pw", 7), ("nimble_backward_masses_pw", 8),
                              ("nimble_backward_inertia_pw", 8), ("nimble_jacobians_pw", 7),
                              ("nimble_constraint_force_jacobians_pw", 7)):
            f = getattr(L, name)
            f.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * buffers + [C.c_void_p]
            f.restype = C.c_int
        for name, argtypes in (list(EXT_PROTOTYPES.items()) + list(ID_PROTOTYPES.items())
                               + list(ID_INERTIA_PROTOTYPES.items()) + list(CID_PROTOTYPES.items())):
            f = getattr(L, name)
            f.argtypes = argtypes
            f.restype = C.c_int
        L.nimble_num_collision_pairs.restype = C.c_int32
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise RuntimeError(f"nimble_amd error {rc}: {lib().nimble_last_error().decode()}")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("nimblephysics_amd runs on the ROCm device only; got a CPU tensor")
        if t is not None and t.dtype.is_floating_point and str(t.dtype) != "torch.float64":
            raise TypeError("nimblephysics_amd computes in float64 (the reference's s_t); got " + str(t.dtype))


# snapshot header (csrc/pool_sizes.h) and status bits (csrc/contact.cuh)
SN_NCON, SN_M, SN_NC, SN_NU, SN_CFM, SN_STATUS = 0, 1, 2, 3, 4, 5
MAX_CONTACTS = 42
MAX_LCP = 3 * MAX_CONTACTS  # include/nimble_amd.h NIMBLE_MAX_LCP
CREC, EDGE_REC, SN_ROWREC = 13, 12, 12  # csrc/pool_sizes.h


def snapshot_layout(n: int, timing: bool = False) -> dict:
    """Per-world snapshot offsets (doubles) of csrc/pool_sizes.h for a model
    with n dofs: header, contact records, row records, f_c, v_f, y_f, the
    backward blocks (A_c, A_c_ub_E, pinv(Q)^T, Q), EDGE metadata, the
    stage-timing build's stamps (`timing`: 128 doubles, ahead of the
    workspace) and the start of the HBM workspace.  tests/test_wave_emu.py
    checks it against the header."""
    a8 = lambda x: ((x + 7) // 8) * 8
    L = {"contacts": 16}
    L["rows"] = L["contacts"] + MAX_CONTACTS * CREC
    L["fc"] = L["rows"] + MAX_LCP * SN_ROWREC
    L["vf"] = L["fc"] + MAX_LCP
    L["yf"] = L["vf"] + n
    L["ac"] = a8(L["yf"] + n)
    L["acube"] = L["ac"] + n * MAX_LCP
    L["pt"] = L["acube"] + n * MAX_LCP
    L["q"] = L["pt"] + MAX_LCP * MAX_LCP
    L["edge"] = L["q"] + MAX_LCP * MAX_LCP
    L["stamps"] = a8(L["edge"] + MAX_CONTACTS * EDGE_REC)
    L["workspace"] = L["stamps"] + (128 if timing else 0)
    return L
SN_FC = 16 + 13 * MAX_CONTACTS + 12 * MAX_LCP  # NIMBLE_SNAPSHOT_FC: clamping impulses f_c
ST_CONTACT_OVERFLOW, ST_UNSUPPORTED_SHAPE, ST_DROPPED_OVERFLOW, ST_REDUCED, ST_LCP_TOO_LARGE = 1, 2, 4, 8, 16
ST_PROTOCOL = 64  # a wait between a world's two waves hit the kernel's deadlock guard
ST_DIVERGES = ST_CONTACT_OVERFLOW | ST_UNSUPPORTED_SHAPE | ST_DROPPED_OVERFLOW | ST_LCP_TOO_LARGE | ST_PROTOCOL
SN_PIVOTS, SN_SWEEPS, SN_SOLVER_FLOPS = 9, 10, 11  # the LCP solvers' executed work (include/nimble_amd.h)
MAX_SOLVED_LCP = 128  # include/nimble_amd.h NIMBLE_MAX_SOLVED_LCP (two rows per lane above 64)


class ContactCapacityError(RuntimeError):
    """A world's contact set does not fit the batched path (more contacts than
    NIMBLE_MAX_CONTACTS, a shape pair without a collider, or an overflowing
    dropped-contact list): its step would differ from the reference's."""


def status_message(bits: int) -> str:
    why = []
    if bits & ST_CONTACT_OVERFLOW:
        why.append("more contacts than NIMBLE_MAX_CONTACTS")
    if bits & ST_UNSUPPORTED_SHAPE:
        why.append("a shape pair without a collider on this path")
    if bits & ST_DROPPED_OVERFLOW:
        why.append("dropped-contact list overflow")
    if bits & ST_LCP_TOO_LARGE:
        why.append(f"more than {MAX_SOLVED_LCP} LCP rows")
    if bits & ST_PROTOCOL:
        why.append("the kernel's two-wave deadlock guard expired (step finished on one wave)")
    return ", ".join(why)


class DeviceWorld:
    """A world model uploaded to one device (nimble_world_create)."""

    def __init__(self, world, device_index: int = 0):
        L = lib()
        desc, keep = world.desc()
        self._keep = keep
        h = C.c_void_p()
        _check(L.nimble_world_create(C.byref(desc), C.byref(h)))
        self.h = h
        self.device_index = int(device_index)
        self.n = world.getNumDofs()
        self.nb = int(desc.num_bodies)
        self.snapshot_doubles = int(L.nimble_snapshot_doubles(h))
        self.cache_doubles = int(L.nimble_lcp_cache_doubles(h))
        self.num_pairs = int(L.nimble_num_collision_pairs(h))

    def close(self):
        if self.h:
            lib().nimble_world_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _on_my_device(self, *tensors):
        for t in tensors:
            if t is not None and t.device.index != self.device_index:
                raise RuntimeError(f"tensor on {t.device}, world model uploaded to cuda:{self.device_index}")

    def _shapes(self, B, state=None, forces=None, snapshot=None, cache=None):
        n = self.n
        if state is not None and tuple(state.shape) != (B, 2 * n):
            raise ValueError(f"state shape {tuple(state.shape)} != ({B}, {2 * n})")
        if forces is not None and tuple(forces.shape) != (B, n):
            raise ValueError(f"forces shape {tuple(forces.shape)} != ({B}, {n})")
        if snapshot is not None and (snapshot.shape[0] < B or snapshot.shape[1] != self.snapshot_doubles):
            raise ValueError(f"snapshot shape {tuple(snapshot.shape)}: this world needs [{B}, {self.snapshot_doubles}]")
        if cache is not None and (cache.shape[0] < B or cache.shape[1] != self.cache_doubles):
            raise ValueError(f"LCP cache shape {tuple(cache.shape)}: this world needs [{B}, {self.cache_doubles}]")
        for t in (state, forces, snapshot, cache):
            if t is not None and not t.is_contiguous():
                raise ValueError("nimblephysics_amd buffers must be contiguous")

    def _inertia(self, B, body_inertia):
        """Checks the optional per-world parameter array (include/nimble_amd.h
        body_inertia: [B, num_bodies, 10] float64, INERTIA_FULL order per
        body) before anything else is looked at; None selects the model's
        own parameters."""
        t = body_inertia
        if t is None:
            return
        if tuple(t.shape) != (B, self.nb, 10):
            raise ValueError(f"body_inertia shape {tuple(t.shape)} != ({B}, {self.nb}, 10)")
        if str(t.dtype) != "torch.float64":
            raise TypeError("body_inertia must be float64 (the reference's s_t); got " + str(t.dtype))
        if not t.is_contiguous():
            raise ValueError("nimblephysics_amd buffers must be contiguous")

    def _wrench(self, B, body_wrench, wrench_frame, grad_wrench=None, rows=None):
        """Checks the optional external body wrenches (include/nimble_amd.h
        body_wrench: [B, num_bodies, 6] float64, [torque xyz, force xyz] per
        body in device-model order) and the output for their gradient;
        returns the frame flag.  None: no wrench."""
        flag = wrench_frame_flag(wrench_frame)
        t = body_wrench
        if t is None:
            if grad_wrench is not None:
                raise ValueError("grad_wrench given without body_wrench")
            return flag
        if tuple(t.shape) != (B, self.nb, 6):
            raise ValueError(f"body_wrench shape {tuple(t.shape)} != ({B}, {self.nb}, 6)")
        if str(t.dtype) != "torch.float64":
            raise TypeError("body_wrench must be float64 (the reference's s_t); got " + str(t.dtype))
        if not t.is_contiguous():
            raise ValueError("nimblephysics_amd buffers must be contiguous")
        if grad_wrench is not None:
            want = (B, self.nb, 6) if rows is None else (B, rows, self.nb, 6)
            if tuple(grad_wrench.shape) != want or not grad_wrench.is_contiguous():
                raise ValueError(f"grad_wrench shape {tuple(grad_wrench.shape)} != {want}")
            if str(grad_wrench.dtype) != "torch.float64":
                raise TypeError("grad_wrench must be float64; got " + str(grad_wrench.dtype))
        return flag

    def status(self, snapshot):
        """Status bits per world ([B] int32, device) of the forward that wrote
        `snapshot`; zeros for models without collision pairs."""
        import torch
        if self.num_pairs == 0:
            return torch.zeros(snapshot.shape[0], dtype=torch.int32, device=snapshot.device)
        return snapshot[:, SN_STATUS].to(torch.int32)

    def forward(self, state, forces, lcp_cache, next_state, snapshot, stream_ptr: int, body_inertia=None,
                body_wrench=None, wrench_frame="world"):
        """nimble_forward; with `body_inertia` [B, num_bodies, 10] every world
        steps with its own body parameters (nimble_forward_pw), and the
        backward / Jacobian calls on its snapshot take the same tensor.  With
        `body_wrench` [B, num_bodies, 6] the bodies are pushed by those
        wrenches, given in `wrench_frame` (nimble_forward_ext); the other
        calls on the snapshot take them too.  (Without: nothing but this test
        is added to the path, which benchmarks time from the host side.)"""
        if body_wrench is not None:
            return self._ext("forward", state, forces, (lcp_cache, next_state, snapshot), stream_ptr, body_inertia,
                             body_wrench, wrench_frame)
        B = state.shape[0]
        self._inertia(B, body_inertia)
        _require_device(state, forces, lcp_cache, next_state, snapshot, body_inertia)
        self._on_my_device(state, forces, lcp_cache, next_state, snapshot, body_inertia)
        self._shapes(B, state, forces, snapshot, lcp_cache)
        if body_inertia is not None:
            _check(lib().nimble_forward_pw(self.h, B, _ptr(state), _ptr(forces), _ptr(lcp_cache), _ptr(next_state),
                                           _ptr(snapshot), _ptr(body_inertia), C.c_void_p(stream_ptr)))
            return
        _check(lib().nimble_forward(self.h, B, _ptr(state), _ptr(forces), _ptr(lcp_cache), _ptr(next_state),
                                    _ptr(snapshot), C.c_void_p(stream_ptr)))

    def backward(self, state, forces, snapshot, grad_next, grad_state, grad_forces, stream_ptr: int,
                 body_inertia=None, body_wrench=None, wrench_frame="world", grad_wrench=None):
        """nimble_backward; `grad_wrench` [B, num_bodies, 6] (with
        `body_wrench`) receives the gradient with respect to the wrenches, in
        their frame (nimble_backward_ext)."""
        if body_wrench is not None or grad_wrench is not None:
            return self._ext("backward", state, forces, (snapshot, grad_next, grad_state, grad_forces), stream_ptr,
                             body_inertia, body_wrench, wrench_frame, grad_wrench)
        B = state.shape[0]
        self._inertia(B, body_inertia)
        _require_device(state, forces, snapshot, grad_next, grad_state, grad_forces, body_inertia)
        self._on_my_device(state, forces, snapshot, grad_next, grad_state, grad_forces, body_inertia)
        self._shapes(B, state, forces, snapshot)
        self._shapes(B, grad_next, grad_forces)
        self._shapes(B, grad_state)
        if body_inertia is not None:
            _check(lib().nimble_backward_pw(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot), _ptr(grad_next),
                                            _ptr(grad_state), _ptr(grad_forces), _ptr(body_inertia),
                                            C.c_void_p(stream_ptr)))
            return
        _check(lib().nimble_backward(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot), _ptr(grad_next),
                                     _ptr(grad_state), _ptr(grad_forces), C.c_void_p(stream_ptr)))

    def backward_masses(self, state, forces, snapshot, grad_next, grad_state, grad_forces, grad_masses,
                        stream_ptr: int, body_inertia=None, body_wrench=None, wrench_frame="world"):
        """backward() plus dL/d(body masses) [B, num_bodies] (nimble_backward_masses)."""
        if body_wrench is not None:
            if tuple(grad_masses.shape) != (state.shape[0], self.nb) or not grad_masses.is_contiguous():
                raise ValueError(f"grad_masses shape {tuple(grad_masses.shape)} != ({state.shape[0]}, {self.nb})")
            return self._ext("backward_masses", state, forces, (snapshot, grad_next, grad_state, grad_forces,
                                                                grad_masses), stream_ptr, body_inertia, body_wrench,
                             wrench_frame)
        B = state.shape[0]
        self._inertia(B, body_inertia)
        _require_device(state, forces, snapshot, grad_next, grad_state, grad_forces, grad_masses, body_inertia)
        self._on_my_device(state, forces, snapshot, grad_next, grad_state, grad_forces, grad_masses, body_inertia)
        self._shapes(B, state, forces, snapshot)
        self._shapes(B, grad_next, grad_forces)
        self._shapes(B, grad_state)
        if tuple(grad_masses.shape) != (B, self.nb) or not grad_masses.is_contiguous():
            raise ValueError(f"grad_masses shape {tuple(grad_masses.shape)} != ({B}, {self.nb})")
        if body_inertia is not None:
            _check(lib().nimble_backward_masses_pw(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot),
                                                   _ptr(grad_next), _ptr(grad_state), _ptr(grad_forces),
                                                   _ptr(grad_masses), _ptr(body_inertia), C.c_void_p(stream_ptr)))
            return
        _check(lib().nimble_backward_masses(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot), _ptr(grad_next),
                                            _ptr(grad_state), _ptr(grad_forces), _ptr(grad_masses),
                                            C.c_void_p(stream_ptr)))

    def backward_inertia(self, state, forces, snapshot, grad_next, grad_state, grad_forces, grad_inertia,
                         stream_ptr: int, body_inertia=None, body_wrench=None, wrench_frame="world"):
        """backward() plus dL/d(body inertia parameters) [B, num_bodies, 10] in
        INERTIA_FULL order (mass, COM xyz, Ixx Iyy Izz Ixy Ixz Iyz;
        nimble_backward_inertia): with `body_inertia`, the gradient with
        respect to that array."""
        if body_wrench is not None:
            if tuple(grad_inertia.shape) != (state.shape[0], self.nb, 10) or not grad_inertia.is_contiguous():
                raise ValueError(f"grad_inertia shape {tuple(grad_inertia.shape)} != ({state.shape[0]}, {self.nb}, 10)")
            return self._ext("backward_inertia", state, forces, (snapshot, grad_next, grad_state, grad_forces,
                                                                 grad_inertia), stream_ptr, body_inertia, body_wrench,
                             wrench_frame)
        B = state.shape[0]
        self._inertia(B, body_inertia)
        _require_device(state, forces, snapshot, grad_next, grad_state, grad_forces, grad_inertia, body_inertia)
        self._on_my_device(state, forces, snapshot, grad_next, grad_state, grad_forces, grad_inertia, body_inertia)
        self._shapes(B, state, forces, snapshot)
        self._shapes(B, grad_next, grad_forces)
        self._shapes(B, grad_state)
        if tuple(grad_inertia.shape) != (B, self.nb, 10) or not grad_inertia.is_contiguous():
            raise ValueError(f"grad_inertia shape {tuple(grad_inertia.shape)} != ({B}, {self.nb}, 10)")
        if body_inertia is not None:
            _check(lib().nimble_backward_inertia_pw(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot),
                                                    _ptr(grad_next), _ptr(grad_state), _ptr(grad_forces),
                                                    _ptr(grad_inertia), _ptr(body_inertia), C.c_void_p(stream_ptr)))
            return
        _check(lib().nimble_backward_inertia(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot), _ptr(grad_next),
                                             _ptr(grad_state), _ptr(grad_forces), _ptr(grad_inertia),
                                             C.c_void_p(stream_ptr)))

    def _ext(self, mode, state, forces, buffers, stream_ptr, body_inertia, body_wrench, wrench_frame,
             grad_wrench=None, wrench_jacobian=False):
        """The calls with external body wrenches (the `_ext` entry points):
        `mode` names the wrapper, `buffers` its tensors after state and forces
        in the entry point's order.  The Jacobian modes allocate their
        outputs as the wrappers without wrenches do."""
        import torch
        B = state.shape[0]
        n = self.n
        self._inertia(B, body_inertia)
        frame = self._wrench(B, body_wrench, wrench_frame, grad_wrench)
        _require_device(state, forces, *buffers, body_inertia, body_wrench, grad_wrench)
        self._on_my_device(state, forces, *buffers, body_inertia, body_wrench, grad_wrench)
        L = lib()
        stream = C.c_void_p(stream_ptr)
        tail = (_ptr(body_inertia), _ptr(body_wrench), frame)
        if mode == "forward":
            lcp_cache, next_state, snapshot = buffers
            self._shapes(B, state, forces, snapshot, lcp_cache)
            _check(L.nimble_forward_ext(self.h, B, _ptr(state), _ptr(forces), _ptr(lcp_cache), _ptr(next_state),
                                        _ptr(snapshot), *tail, stream))
            return None
        if mode in ("jacobians", "constraint_force_jacobians"):
            snapshot, = buffers
            self._shapes(B, state, forces, snapshot)
            wsd = int(L.nimble_jacobian_workspace_doubles(self.h, B))
            ws = torch.empty(wsd, dtype=torch.float64, device=state.device) if wsd > 0 else None
            if mode == "jacobians":
                J = torch.empty((B, 2 * n, 2 * n), dtype=torch.float64, device=state.device)
                F = torch.empty((B, 2 * n, n), dtype=torch.float64, device=state.device)
                W = torch.empty((B, 2 * n, self.nb, 6), dtype=torch.float64, device=state.device) \
                    if wrench_jacobian else None
                _check(L.nimble_jacobians_ext(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot), _ptr(J), _ptr(F),
                                              _ptr(ws), *tail, _ptr(W), stream))
                return (J, F, W) if wrench_jacobian else (J, F)
            Js = torch.empty((B, MAX_LCP, 2 * n), dtype=torch.float64, device=state.device)
            Jf = torch.empty((B, MAX_LCP, n), dtype=torch.float64, device=state.device)
            _check(L.nimble_constraint_force_jacobians_ext(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot),
                                                           _ptr(Js), _ptr(Jf), _ptr(ws), *tail, stream))
            return Js, Jf
        snapshot, grad_next, grad_state, grad_forces = buffers[:4]
        self._shapes(B, state, forces, snapshot)
        self._shapes(B, grad_next, grad_forces)
        self._shapes(B, grad_state)
        head = (self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot), _ptr(grad_next), _ptr(grad_state),
                _ptr(grad_forces))
        if mode == "backward":
            _check(L.nimble_backward_ext(*head, *tail, _ptr(grad_wrench), stream))
        elif mode == "backward_masses":
            _check(L.nimble_backward_masses_ext(*head, _ptr(buffers[4]), *tail, stream))
        else:
            _check(L.nimble_backward_inertia_ext(*head, _ptr(buffers[4]), *tail, stream))
        return None

    def _id_args(self, state, ddq, body_inertia, body_wrench, wrench_frame, grad_wrench=None, **named):
        """Checks shared by inverse_dynamics / inverse_dynamics_backward:
        shapes, dtypes and the frame first (no device needed for those), then
        that everything is on this world's device; `named` are further [B, n]
        (or, by name, other) buffers.  Returns (B, frame flag)."""
        n = self.n
        if state.dim() != 2 or state.shape[1] != 2 * n:
            raise ValueError(f"state shape {tuple(state.shape)} != (batch, {2 * n})")
        B = state.shape[0]
        want = {"mass_matrix": (B, n, n), "grad_state": (B, 2 * n), "grad_inertia": (B, self.nb, 10),
                "jacobian": (B, n, self.nb, 10)}
        for name, t in (("state", state), ("ddq", ddq)) + tuple(named.items()):
            if t is None:
                continue
            shape = want.get(name, (B, 2 * n) if name == "state" else (B, n))
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} shape {tuple(t.shape)} != {shape}")
            if str(t.dtype) != "torch.float64":
                raise TypeError(f"{name} must be float64 (the reference's s_t); got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError("nimblephysics_amd buffers must be contiguous")
        self._inertia(B, body_inertia)
        frame = self._wrench(B, body_wrench, wrench_frame, grad_wrench)
        every = (state, ddq, body_inertia, body_wrench, grad_wrench) + tuple(named.values())
        _require_device(*every)
        self._on_my_device(*every)
        return B, frame

    def inverse_dynamics(self, state, ddq, tau, stream_ptr: int, body_inertia=None, body_wrench=None,
                         wrench_frame="world", mass_matrix=None, bias=None):
        """nimble_inverse_dynamics: tau [B, n] = M a + C - tau_ext + D v +
        K (q - q0 + dt v) for state [B, 2n] and ddq [B, n]; `mass_matrix`
        [B, n, n] and `bias` [B, n] (C with gravity alone) are filled when
        given.  `body_inertia` / `body_wrench` / `wrench_frame` as for
        forward()."""
        B, frame = self._id_args(state, ddq, body_inertia, body_wrench, wrench_frame, tau=tau,
                                 mass_matrix=mass_matrix, bias=bias)
        _check(lib().nimble_inverse_dynamics(self.h, B, _ptr(state), _ptr(ddq), _ptr(body_inertia), _ptr(body_wrench),
                                             frame, _ptr(tau), _ptr(mass_matrix), _ptr(bias),
                                             C.c_void_p(stream_ptr)))

    def inverse_dynamics_backward(self, state, ddq, grad_tau, grad_state, grad_ddq, stream_ptr: int,
                                  body_inertia=None, body_wrench=None, wrench_frame="world", grad_wrench=None,
                                  grad_inertia=None):
        """nimble_inverse_dynamics_backward: the vector-Jacobian product with
        grad_tau [B, n] into grad_state [B, 2n], grad_ddq [B, n] and (with
        `body_wrench`) grad_wrench [B, num_bodies, 6], in the wrench's frame.
        With `grad_inertia` [B, num_bodies, 10]
        (nimble_invdyn_backward_inertia) also the gradient in every
        device-model body's inertial parameters, INERTIA_FULL order."""
        B, frame = self._id_args(state, ddq, body_inertia, body_wrench, wrench_frame, grad_wrench,
                                 grad_tau=grad_tau, grad_state=grad_state, grad_ddq=grad_ddq,
                                 grad_inertia=grad_inertia)
        head = (self.h, B, _ptr(state), _ptr(ddq), _ptr(body_inertia), _ptr(body_wrench), frame, _ptr(grad_tau),
                _ptr(grad_state), _ptr(grad_ddq), _ptr(grad_wrench))
        if grad_inertia is not None:
            _check(lib().nimble_invdyn_backward_inertia(*head, _ptr(grad_inertia), C.c_void_p(stream_ptr)))
        else:
            _check(lib().nimble_inverse_dynamics_backward(*head, C.c_void_p(stream_ptr)))

    def inverse_dynamics_inertia_jacobian(self, state, ddq, jacobian, stream_ptr: int, body_inertia=None):
        """nimble_invdyn_inertia_jacobian: d tau / d theta into
        `jacobian` [B, n, num_bodies, 10] (device-model bodies, INERTIA_FULL
        order) for state [B, 2n] and ddq [B, n]; every element is written."""
        if jacobian is None:
            raise ValueError("jacobian is required")
        B, _ = self._id_args(state, ddq, body_inertia, None, "world", jacobian=jacobian)
        _check(lib().nimble_invdyn_inertia_jacobian(self.h, B, _ptr(state), _ptr(ddq), _ptr(body_inertia),
                                                              _ptr(jacobian), C.c_void_p(stream_ptr)))

    def contact_inverse_dynamics(self, state, ddq, contact_bodies, tau, contact_wrenches, stream_ptr: int,
                                 wrench_guesses=None, body_inertia=None, body_wrench=None, wrench_frame="world"):
        """nimble_contact_inverse_dynamics: for state [B, 2n], ddq [B, n] and
        the k device-model body indices `contact_bodies` (distinct, all of one
        skeleton with a free root joint), tau [B, n] with the root's six rows
        0 and contact_wrenches [B, k, 6] in each body's own frame;
        `wrench_guesses` [B, k, 6] selects the solution nearest them.
        `body_inertia` / `body_wrench` / `wrench_frame` as for
        inverse_dynamics()."""
        bodies = [int(b) for b in contact_bodies]
        k = len(bodies)
        if k < 1 or k > MAX_CONTACT_BODIES:
            raise ValueError(f"{k} contact bodies: 1 .. {MAX_CONTACT_BODIES} are supported")
        if min(bodies) < 0 or max(bodies) >= self.nb:
            raise ValueError(f"contact body index outside 0 .. {self.nb - 1}: {bodies}")
        if len(set(bodies)) != k:
            raise ValueError(f"duplicate contact body: {bodies}")
        if state.dim() != 2:
            raise ValueError(f"state shape {tuple(state.shape)} != (batch, {2 * self.n})")
        B = state.shape[0]
        for name, t in (("contact_wrenches", contact_wrenches), ("wrench_guesses", wrench_guesses)):
            if t is None:
                continue
            if tuple(t.shape) != (B, k, 6):
                raise ValueError(f"{name} shape {tuple(t.shape)} != {(B, k, 6)}")
            if str(t.dtype) != "torch.float64":
                raise TypeError(f"{name} must be float64 (the reference's s_t); got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError("nimblephysics_amd buffers must be contiguous")
        _, frame = self._id_args(state, ddq, body_inertia, body_wrench, wrench_frame, tau=tau)
        _require_device(contact_wrenches, wrench_guesses)
        self._on_my_device(contact_wrenches, wrench_guesses)
        idx = (C.c_int32 * k)(*bodies)
        _check(lib().nimble_contact_inverse_dynamics(self.h, B, _ptr(state), _ptr(ddq), _ptr(body_inertia),
                                                     _ptr(body_wrench), frame, k, idx, _ptr(wrench_guesses),
                                                     _ptr(tau), _ptr(contact_wrenches), C.c_void_p(stream_ptr)))

    def jacobians(self, state, forces, snapshot, stream_ptr: int, body_inertia=None, body_wrench=None,
                  wrench_frame="world", wrench_jacobian=False):
        """(d next_state / d state [B, 2n, 2n], d next_state / d forces
        [B, 2n, n]) of the forward that wrote `snapshot` (nimble_jacobians).
        `wrench_jacobian=True` (with `body_wrench`): a third result,
        d next_state / d body_wrench [B, 2n, num_bodies, 6]
        (nimble_jacobians_ext)."""
        import torch
        if wrench_jacobian and body_wrench is None:
            raise ValueError("wrench_jacobian needs body_wrench")
        if body_wrench is not None:
            return self._ext("jacobians", state, forces, (snapshot,), stream_ptr, body_inertia, body_wrench,
                             wrench_frame, wrench_jacobian=wrench_jacobian)
        B = state.shape[0]
        self._inertia(B, body_inertia)
        _require_device(state, forces, snapshot, body_inertia)
        self._on_my_device(state, forces, snapshot, body_inertia)
        self._shapes(B, state, forces, snapshot)
        n = self.n
        J = torch.empty((B, 2 * n, 2 * n), dtype=torch.float64, device=state.device)
        F = torch.empty((B, 2 * n, n), dtype=torch.float64, device=state.device)
        wsd = int(lib().nimble_jacobian_workspace_doubles(self.h, B))
        ws = torch.empty(wsd, dtype=torch.float64, device=state.device) if wsd > 0 else None
        if body_inertia is not None:
            _check(lib().nimble_jacobians_pw(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot), _ptr(J), _ptr(F),
                                             _ptr(ws), _ptr(body_inertia), C.c_void_p(stream_ptr)))
            return J, F
        _check(lib().nimble_jacobians(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot), _ptr(J), _ptr(F),
                                      _ptr(ws), C.c_void_p(stream_ptr)))
        return J, F

    def constraint_force_jacobians(self, state, forces, snapshot, stream_ptr: int, body_inertia=None,
                                   body_wrench=None, wrench_frame="world"):
        """(d f_c / d state [B, MAX_LCP, 2n], d f_c / d forces [B, MAX_LCP, n])
        of the forward that wrote `snapshot` (nimble_constraint_force_jacobians;
        rows past each world's clamping count are zero)."""
        import torch
        if body_wrench is not None:
            return self._ext("constraint_force_jacobians", state, forces, (snapshot,), stream_ptr, body_inertia,
                             body_wrench, wrench_frame)
        B = state.shape[0]
        self._inertia(B, body_inertia)
        _require_device(state, forces, snapshot, body_inertia)
        self._on_my_device(state, forces, snapshot, body_inertia)
        self._shapes(B, state, forces, snapshot)
        n = self.n
        Js = torch.empty((B, MAX_LCP, 2 * n), dtype=torch.float64, device=state.device)
        Jf = torch.empty((B, MAX_LCP, n), dtype=torch.float64, device=state.device)
        wsd = int(lib().nimble_jacobian_workspace_doubles(self.h, B))
        ws = torch.empty(wsd, dtype=torch.float64, device=state.device) if wsd > 0 else None
        if body_inertia is not None:
            _check(lib().nimble_constraint_force_jacobians_pw(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot),
                                                              _ptr(Js), _ptr(Jf), _ptr(ws), _ptr(body_inertia),
                                                              C.c_void_p(stream_ptr)))
            return Js, Jf
        _check(lib().nimble_constraint_force_jacobians(self.h, B, _ptr(state), _ptr(forces), _ptr(snapshot),
                                                       _ptr(Js), _ptr(Jf), _ptr(ws), C.c_void_p(stream_ptr)))
        return Js, Jf


def contact_flop_estimate(world, rows: float, clamping: float) -> dict:
    """Algorithmic fp64 FLOPs per world of the contact stage for `rows` LCP
    rows of which `clamping` clamp (batch averages), FMA = 2.  Forward: J^T
    columns, Y = L^-1 J^T, A = Y^T Y, b, guess + standardisation COD solves,
    validity checks, impulses, and the backward precompute (A_c, A_c_ub_E, Q,
    COD + pinv(Q), rank check).  Backward: the nine Minv products (two batched
    Cholesky solves), the clamping-space vector chain, per-row G vectors,
    chain twists, grouped contact-geometry terms and the M-derivative fields.
    Iterative fallbacks (Dantzig pivots, PGS sweeps) are not counted."""
    d = world.desc_arrays()
    nb, n = int(d["num_bodies"]), int(d["num_dofs"])
    m, c = float(rows), float(clamping)
    if m <= 0:
        return {"forward": 0.0, "backward": 0.0}
    cod = lambda k: 4.0 / 3.0 * k ** 3 + 4.0 * k * k  # noqa: E731
    fwd = (14 * n * m + n * n * m + m * m * n + 2 * n * m + 2 * cod(m) + 4 * m * m + 2 * n * m + n * n
           + 2 * 14 * n * c + 2 * c * c + cod(c) + 4 * c ** 3 + 2 * c ** 3)
    groups = 2.0
    bwd = (18 * n * n + 12 * 2 * n * c + 6 * 2 * c * c + 12 * m * n + 24 * m * n
           + groups * (12 * m * n + 18 * nb * n) + 8 * nb * (12 * n + 100) + 20 * n)
    return {"forward": float(fwd), "backward": float(bwd)}


def flop_estimate(world, rows: float = 0.0, clamping: float = 0.0) -> dict:
    """Algorithmic fp64 FLOPs per world for one launch of each kernel, counted
    from the implemented algorithm's loop structure (FMA = 2 FLOPs): forward =
    kinematics, world-frame composites, CRBA mass matrix, Cholesky + solve
    (+ contact stage); backward = accelerations at a*, derivative composites,
    one closed-form dID/dq and dC/dv column per dof (only related body pairs)
    and two solves (+ contact terms)."""
    d = world.desc_arrays()
    nb, n = int(d["num_bodies"]), int(d["num_dofs"])
    parent = list(d["parent"])
    jt = list(d["joint_type"])
    ndof = [{0: 0, 1: 1, 2: 1, 3: 6, 4: 3, 5: 3}[int(t)] for t in jt]
    anc = []
    for b in range(nb):
        s = {b}
        p = parent[b]
        while p >= 0:
            s.add(p)
            p = parent[p]
        anc.append(s)
    dof_body = []
    for b in range(nb):
        dof_body += [b] * ndof[b]
    kin = sum(330 + 60 * ndof[b] for b in range(nb))
    comp = nb * 330 + nb * 42
    related_pairs = sum(1 for j in range(n) for k in range(j + 1)
                        if dof_body[k] in anc[dof_body[j]] or dof_body[j] in anc[dof_body[k]])
    mass = related_pairs * 84 + n * 12
    chol = n ** 3 / 3.0 + n ** 2
    solve = 2.0 * n * n
    fwd = kin + comp + mass + chol + solve + 10 * n
    dcomp = nb * 1800 + nb * 126
    lanes = 0.0
    for k in range(n):
        b = dof_body[k]
        lanes += 1020
        for c in range(nb):
            if ndof[c] == 0:
                continue
            if b in anc[c]:
                lanes += (1020 if c != b else 0) + 80 * ndof[c]
            elif c in anc[b]:
                lanes += 50 * ndof[c]
    # the backward reuses the forward's kinematics, composite inertias and
    # Cholesky factor (snapshot dynamics cache): accelerations + derivative
    # composites + the per-direction columns + two solves
    accel = nb * n * 30
    bwd = accel + dcomp + lanes + 2 * solve + 20 * n
    c = contact_flop_estimate(world, rows, clamping)
    return {"forward": float(fwd + c["forward"]), "backward": float(bwd + c["backward"])}
