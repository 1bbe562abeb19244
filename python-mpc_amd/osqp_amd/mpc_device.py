"""Device-resident MPC data path around the solver.

The reference's incremental dynamic-bicycle MPC (Control/MPC/mpc_dynamics.py:main)
does, per control step and in Python:

  Xr = reference_search(path_x, path_y, pred_x~, dt, N)            :44-90   (F3)
  Ad_k, Bd_k, gd_k = vehicle.get_dynamics_model(pred_x~[:, k])      vehicle_models.py:52-340 (F2)
  pred_x~, pred_du = mpc_increment(Ad, Bd, gd, x~, Xr, ...)         :281-432 (F1 + the solve)
  plant step + horizon shift                                        :578-617 (F3)

This module runs the same steps for B vehicles at once on the MI355X through the
C ABI of include/mpcqp.h (mpcqp_linearise_device, mpcqp_incr_*,
mpcqp_reference_search_device) and the batched solver (DeviceBatch).  Arrays are
torch tensors on the device; nothing is copied to the host inside a step.

KinematicMPC is the same loop on the kinematic bicycle, Control/MPC/mpc_incre_kine_func.py:
simulate (:223-436), with its trajectory record and stop rule (mpcqp_kin_linearise_device,
mpcqp_kin_reference_search_device, mpcqp_kin_shift_device).

LTVLayout is the LTV MPC in the inputs themselves (mpc__, mpc_dynamics.mpc, mpc_'s corridor;
mpcqp_ltv_*), and KinematicLTVMPC the closed loop of Control/MPC/mpc_kinematics_pred_matrix.py:
main (:355-563) on it (mpcqp_kin_rollout_device, mpcqp_kin_ltv_shift_device).

LaneChangeMPC is the closed loop of Control/MPC/mpc_increment_kinematics_pred_matrix.py:main
(:281-476, the double lane change) on IncrementalLayout, over a bank of paths with one selected per
vehicle (mpcqp_kin_reference_search_paths_device, mpcqp_lane_tail_device); KinematicFrozenMPC the
closed loop of Control/MPC/mpc_kinematics.py:main (:268-461) on LTVLayout with one linearisation per
step on every stage (mpcqp_kin_frozen_tail_device).

LateralMPC is the closed loop of vehicle_lateral_mpc_slack_increment.py (:123-269), the one loop
that keeps a problem alive: one setup, then per step LateralAssembler -> DeviceBatch.update ->
warm-started DeviceBatch.solve -> mpcqp_lti_step_device.

Wherever a function or a class here takes ``veh`` (a Vehicle or KinVehicle struct: one car for the
whole batch) it also takes a Fleet / KinFleet: a table with one car per vehicle of the batch
(mpcqp_fleet_create and the `_fleet` twins of the entry points).  LateralMPC, whose
model is fixed at setup, takes neither.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sparse

from . import DeviceBatch, _check, lib

_P = C.POINTER
vp = C.c_void_p


class Vehicle(C.Structure):
    """Vehicle_Dynamics.__init__ arguments (vehicle_models.py:27-50); dt as in mpc_dynamics.main (0.05)."""
    _fields_ = [(k, C.c_double) for k in ("m", "l_f", "l_r", "width", "length", "C_d", "A_f", "C_roll", "dt")]

    def __init__(self, m=1300, l_f=1.25, l_r=1.40, width=1.78, length=4.25, C_d=0.34, A_f=2.0, C_roll=0.015,
                 dt=0.05):
        super().__init__(m, l_f, l_r, width, length, C_d, A_f, C_roll, dt)


class KinVehicle(C.Structure):
    """Vehicle_Kinematics.__init__ arguments (vehicle_models.py:829-833); dt as in
    mpc_incre_kine_func.simulate (0.02)."""
    _fields_ = [(k, C.c_double) for k in ("l_f", "l_r", "dt")]

    def __init__(self, l_f=1.25, l_r=1.40, dt=0.02):
        super().__init__(l_f, l_r, dt)


class _FleetBase:
    """A batch of different vehicles: one table of model constants, entry b for vehicle b
    (mpcqp_fleet / mpcqp_kin_fleet).  Accepted wherever this module takes ``veh``; the batch must then
    have the fleet's size.  Every vehicle of a fleet has the same dt (``dt``)."""
    _struct = _create = _free = None

    def __init__(self, vehicles, device=0):
        vehicles = list(vehicles)
        if not all(isinstance(v, self._struct) for v in vehicles):
            raise TypeError(f"{type(self).__name__} takes a sequence of {self._struct.__name__}")
        self._h = None
        self._vehicles = (self._struct * max(len(vehicles), 1))(*vehicles)
        self._n = len(vehicles)
        self.device = int(device)
        L = _bind()
        self._release = getattr(L, self._free)  # bound now: __del__ may run while the interpreter shuts down
        h = vp()
        _check(getattr(L, self._create)(self._n, self._vehicles, self.device, C.byref(h)), "fleet_create")
        self._h = h

    @classmethod
    def from_arrays(cls, device=0, **fields):
        """One array or scalar per constructor argument of the vehicle struct, broadcast to the
        fleet's size B (the longest array's); an argument not given takes the struct's default."""
        names = [k for k, _ in cls._struct._fields_]
        bad = sorted(set(fields) - set(names))
        if bad:
            raise TypeError(f"unknown field(s) {', '.join(bad)}; {cls._struct.__name__} has {', '.join(names)}")
        cols = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in fields.values()), np.zeros(1))[:-1]
        if any(c.ndim != 1 for c in cols):
            raise ValueError("every field must be a scalar or a 1-D array")
        return cls([cls._struct(**{k: float(c[b]) for k, c in zip(fields, cols)}) for b in range(cols[0].shape[0])]
                   if cols else [cls._struct()], device=device)

    def __len__(self):
        return self._n

    def __getitem__(self, b):
        if not -self._n <= b < self._n:
            raise IndexError(b)
        v = self._vehicles[b % self._n]
        return self._struct(*(getattr(v, k) for k, _ in self._struct._fields_))

    @property
    def dt(self):
        return self._vehicles[0].dt

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._release(h)


class Fleet(_FleetBase):
    """B dynamic bicycles (Vehicle structs)."""
    _struct, _create, _free = Vehicle, "mpcqp_fleet_create", "mpcqp_fleet_free"

    def constants(self):
        """(B, 13): each vehicle's derived constants as the kernels read them, in the order
        (m, l_f, l_r, Iz, dt, roh C_d A_f, C_roll m 9.81, B_f, C_f, D_f, B_r, C_r, D_r)."""
        out = np.empty((self._n, 13))
        for b in range(self._n):
            _check(_bind().mpcqp_fleet_constants(self._h, b, _np_ptr(out[b])), "fleet_constants")
        return out

    def constants_vjp(self, gK):
        """(B, 13) cotangent of ``constants()`` -> (B, 9) of the constructor arguments, in the
        struct's field order (m, l_f, l_r, width, length, C_d, A_f, C_roll, dt): the chain through
        each vehicle's derivation (mpcqp_vehicle_constants_vjp; host only).  gK: an array, or a
        tensor on any device; the result is a float64 numpy array."""
        gK = np.ascontiguousarray(gK.detach().cpu().numpy() if hasattr(gK, "detach") else gK, dtype=np.float64)
        if gK.shape != (self._n, 13):
            raise ValueError(f"gK must be ({self._n}, 13)")
        out = np.empty((self._n, 9))
        for b in range(self._n):
            _check(_bind().mpcqp_vehicle_constants_vjp(C.byref(self._vehicles[b]), _np_ptr(gK[b]), _np_ptr(out[b])),
                   "vehicle_constants_vjp")
        return out


class KinFleet(_FleetBase):
    """B kinematic bicycles (KinVehicle structs)."""
    _struct, _create, _free = KinVehicle, "mpcqp_kin_fleet_create", "mpcqp_kin_fleet_free"

    def constants_vjp(self, gK):
        """The kinematic struct derives nothing: (B, 3) -> (B, 3), the identity."""
        gK = np.array(gK.detach().cpu().numpy() if hasattr(gK, "detach") else gK, dtype=np.float64)
        if gK.shape != (self._n, 3):
            raise ValueError(f"gK must be ({self._n}, 3)")
        return gK


def _entry(name, veh, B):
    """The entry point mpcqp_<name>_device and its vehicle argument; for a fleet the `_fleet` twin
    and the fleet's handle, once its size is known to be the batch's."""
    L = _bind()
    if isinstance(veh, _FleetBase):
        if len(veh) != B:
            raise ValueError(f"{name}: a fleet of {len(veh)} vehicles was given a batch of {B}")
        return getattr(L, f"mpcqp_{name}_fleet_device"), veh._h
    return getattr(L, f"mpcqp_{name}_device"), C.byref(veh)


# structural nonzeros of get_dynamics_model's Ad and Bd (kept under these names here too)
from .mpc import DYN_MASK_A, DYN_MASK_B  # noqa: E402
from .mpc import SLACK_REGIMES, SLACK_SWITCH_STEPS  # noqa: E402  (the slack script's bound schedule)
from .mpc import LANE_PATHS_OF, LANE_SWITCH_STEPS  # noqa: E402  (the lane-change script's path schedule)


def _bind():
    L = lib()
    if getattr(L, "_mpc_bound", False):
        return L
    i64, i32, d = C.c_int64, C.c_int32, C.c_double
    L.mpcqp_linearise_device.argtypes = [_P(Vehicle), i64, i32, vp, i64, i64, vp, i64, i64, vp, vp, vp, i32, vp]
    L.mpcqp_incr_layout_create.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, _P(vp)]
    L.mpcqp_incr_layout_dims.argtypes = [vp, _P(i32), _P(i32), _P(i32), _P(i32)]
    L.mpcqp_incr_layout_pattern.argtypes = [vp] * 9
    L.mpcqp_incr_assemble_device.argtypes = [vp, i64] + [vp] * 10
    L.mpcqp_incr_layout_free.argtypes = [vp]
    L.mpcqp_incr_layout_free.restype = None
    L.mpcqp_reference_search_device.argtypes = [i64, i32, i32, i32, vp, vp, vp, d, vp, i32, vp]
    L.mpcqp_incr_shift_device.argtypes = [vp, _P(Vehicle), i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mpcqp_incr_shift_vjp_device.argtypes = [vp, _P(Vehicle), i64] + [vp] * 14
    L.mpcqp_incr_warm_shift_device.argtypes = [i64, i32, i32, i32, vp, vp, vp, vp, i32, vp]
    L.mpcqp_affine_create.argtypes = [i32, vp, i32, i32, vp, vp, vp, i32, _P(vp)]
    L.mpcqp_affine_apply_device.argtypes = [vp, i64, vp, i32, vp, vp, vp, vp, vp]
    L.mpcqp_affine_free.argtypes = [vp]
    L.mpcqp_affine_free.restype = None
    L.mpcqp_kin_linearise_device.argtypes = [_P(KinVehicle), i64, i32, vp, i64, i64, vp, i64, i64, vp, vp, vp, i32,
                                             vp]
    L.mpcqp_kin_reference_search_device.argtypes = [i64, i32, i32, i32, vp, vp, vp, vp, vp, d, vp, i32, vp]
    L.mpcqp_kin_shift_device.argtypes = [vp, _P(KinVehicle), i64] + [vp] * 11 + [i32, vp, vp]
    L.mpcqp_kin_shift_vjp_device.argtypes = [vp, _P(KinVehicle), i64] + [vp] * 15
    L.mpcqp_ltv_layout_create.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, _P(vp)]
    L.mpcqp_ltv_layout_dims.argtypes = [vp, _P(i32), _P(i32), _P(i32), _P(i32)]
    L.mpcqp_ltv_layout_pattern.argtypes = [vp] * 9
    L.mpcqp_ltv_assemble_device.argtypes = [vp, i64] + [vp] * 12
    L.mpcqp_ltv_layout_free.argtypes = [vp]
    L.mpcqp_ltv_layout_free.restype = None
    L.mpcqp_kin_rollout_device.argtypes = [_P(KinVehicle), i64, i32, vp, vp, vp, vp, i32, vp]
    L.mpcqp_kin_ltv_shift_device.argtypes = [vp, _P(KinVehicle), i64] + [vp] * 12 + [i32, vp, vp]
    L.mpcqp_kin_ltv_shift_vjp_device.argtypes = [vp, _P(KinVehicle), i64] + [vp] * 15
    L.mpcqp_lti_step_device.argtypes = [i64, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp,
                                        vp, vp, i32, vp, i32, vp]
    L.mpcqp_kin_reference_search_paths_device.argtypes = [i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, d, vp, i32,
                                                          vp]
    L.mpcqp_lane_tail_device.argtypes = [vp, _P(KinVehicle), i64] + [vp] * 7 + [i32, vp, vp, vp, vp, vp, i32, vp, vp]
    L.mpcqp_kin_frozen_tail_device.argtypes = [vp, i64] + [vp] * 11 + [i32, vp, vp]
    L.mpcqp_ltv_assemble_w_device.argtypes = [vp, i64] + [vp] * 16
    L.mpcqp_incr_assemble_w_device.argtypes = [vp, i64] + [vp] * 14
    L.mpcqp_ltv_assemble_vjp_device.argtypes = [vp, i64] + [vp] * 21
    L.mpcqp_incr_assemble_vjp_device.argtypes = [vp, i64] + [vp] * 17
    L.mpcqp_affine_vjp_device.argtypes = [vp, i64, vp, vp, vp, vp, vp, i32, vp]
    L.mpcqp_kin_linearise_vjp_device.argtypes = [_P(KinVehicle), i64, i32, vp, i64, i64, vp, i64, i64, vp, vp, vp, vp,
                                                 vp, i32, vp]
    L.mpcqp_linearise_vjp_device.argtypes = [_P(Vehicle), i64, i32, vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, i32,
                                             vp]
    # fleets: every twin has its entry point's argument types with the fleet's handle for the struct
    L.mpcqp_fleet_create.argtypes = L.mpcqp_kin_fleet_create.argtypes = [i64, vp, i32, _P(vp)]
    L.mpcqp_fleet_constants.argtypes = [vp, i64, vp]
    for free in (L.mpcqp_fleet_free, L.mpcqp_kin_fleet_free):
        free.argtypes, free.restype = [vp], None
    for name in ("linearise", "linearise_vjp", "incr_shift", "incr_shift_vjp", "kin_linearise", "kin_linearise_vjp",
                 "kin_shift", "kin_shift_vjp", "kin_rollout", "kin_ltv_shift", "kin_ltv_shift_vjp", "lane_tail"):
        twin = getattr(L, f"mpcqp_{name}_device").argtypes
        getattr(L, f"mpcqp_{name}_fleet_device").argtypes = [
            vp if t in (_P(Vehicle), _P(KinVehicle)) else t for t in twin]
    # gradients with respect to a fleet's constants (fleet form only)
    L.mpcqp_linearise_pvjp_fleet_device.argtypes = L.mpcqp_kin_linearise_pvjp_fleet_device.argtypes = [
        vp, i64, i32, vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, i32, vp]
    L.mpcqp_euler_step_pvjp_fleet_device.argtypes = L.mpcqp_kin_update_pvjp_fleet_device.argtypes = [
        vp, i64, vp, i64, vp, i64, vp, vp, vp, i32, vp]
    L.mpcqp_vehicle_constants_vjp.argtypes = [_P(Vehicle), vp, vp]
    L._mpc_bound = True
    return L


def _p(t):
    return C.c_void_p(t.data_ptr())


def _po(t):
    """_p, or NULL for None (an optional argument of the C ABI)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data)


def _stream(torch, device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _linearise(symbol, veh, x, u, nx):
    """linearise / linearise_kinematics: the model's C entry point on (B, N, nx) states."""
    import torch
    L = _bind()
    squeeze = x.dim() == 2
    if squeeze:
        x, u = x[:, None, :], u[:, None, :]
    B, N = x.shape[0], x.shape[1]
    if x.shape[2] != nx or u.shape[2] != 2 or u.shape[:2] != x.shape[:2]:
        raise ValueError(f"x must be (B, N, {nx}) and u (B, N, 2)")
    if x.stride(2) != 1 or u.stride(2) != 1:
        raise ValueError("the state / input axis must be contiguous")
    kw = dict(dtype=torch.float64, device=x.device)
    fn, v = _entry(symbol, veh, B)
    Ad = torch.empty((B, N, nx, nx), **kw); Bd = torch.empty((B, N, nx, 2), **kw); gd = torch.empty((B, N, nx), **kw)
    _check(fn(v, B, N, _p(x), x.stride(0), x.stride(1), _p(u), u.stride(0), u.stride(1), _p(Ad), _p(Bd), _p(gd),
              x.device.index or 0, _stream(torch, x.device)), symbol)
    if squeeze:
        return Ad[:, 0], Bd[:, 0], gd[:, 0]
    return Ad, Bd, gd


def linearise(veh: Vehicle, x, u, device=0):
    """Batched Vehicle_Dynamics.get_dynamics_model (F2).

    x: (B, N, 6) or (B, 6) float64 device tensor, u: (B, N, 2) or (B, 2) (any strides
    with a contiguous last dimension) -> Ad (B, N, 6, 6), Bd (B, N, 6, 2), gd (B, N, 6)
    (N axis dropped for 2-D inputs).  Inputs are not modified (the reference's
    low-speed guard writes into the caller's view; here it acts on copies)."""
    return _linearise("linearise", veh, x, u, 6)


def _vjp_point(x, u, gAd, gBd, ggd, nx):
    """The point and cotangents of a linearisation's VJP, checked: (x, u) as (B, N, ..) views and
    whether the N axis was added."""
    import torch
    squeeze = x.dim() == 2
    if squeeze:
        x, u = x[:, None, :], u[:, None, :]
    B, N = x.shape[0], x.shape[1]
    if x.shape[2] != nx or u.shape[2] != 2 or u.shape[:2] != x.shape[:2]:
        raise ValueError(f"x must be (B, N, {nx}) and u (B, N, 2)")
    if x.dtype != torch.float64 or u.dtype != torch.float64:
        raise ValueError("x and u must be float64")
    if x.stride(2) != 1 or u.stride(2) != 1:
        raise ValueError("the state / input axis must be contiguous")
    for t, tail in ((gAd, (nx, nx)), (gBd, (nx, 2)), (ggd, (nx,))):
        if t is not None and (t.numel() != B * N * int(np.prod(tail)) or tuple(t.shape[-len(tail):]) != tail or
                              t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError(f"cotangents must be contiguous float64 (B, N, {nx}, {nx}), (B, N, {nx}, 2), "
                             f"(B, N, {nx}) tensors")
    return x, u, squeeze


def _linearise_vjp(symbol, veh, x, u, gAd, gBd, ggd, nx, out=None):
    """linearise_vjp / linearise_kinematics_vjp: the model's C entry point on (B, N, nx) states."""
    import torch
    L = _bind()
    x, u, squeeze = _vjp_point(x, u, gAd, gBd, ggd, nx)
    B, N = x.shape[0], x.shape[1]
    kw = dict(dtype=torch.float64, device=x.device)
    if out is None:
        gx = torch.empty((B, N, nx), **kw); gu = torch.empty((B, N, 2), **kw)
    else:
        gx, gu = out
        for t, w in ((gx, nx), (gu, 2)):
            if tuple(t.shape) != (B, N, w) or t.dtype != torch.float64 or not t.is_contiguous() or t.device != x.device:
                raise ValueError(f"out must be contiguous float64 (B, N, {nx}) and (B, N, 2) tensors on x's device")
    fn, v = _entry(symbol, veh, B)
    _check(fn(v, B, N, _p(x), x.stride(0), x.stride(1), _p(u), u.stride(0), u.stride(1), _po(gAd), _po(gBd),
              _po(ggd), _p(gx), _p(gu), x.device.index or 0, _stream(torch, x.device)), symbol)
    if squeeze:
        return gx[:, 0], gu[:, 0]
    return gx, gu


def linearise_vjp(veh: Vehicle, x, u, gAd, gBd, ggd, out=None):
    """The VJP of linearise (mpcqp_linearise_vjp_device): x (B, N, 6) or (B, 6), u (B, N, 2) or
    (B, 2) as the forward took them (any strides with a contiguous last dimension -- a stage stride
    of 0 included), cotangents gAd (B, N, 6, 6), gBd (B, N, 6, 2), ggd (B, N, 6) contiguous float64
    device tensors, None = zero -> dense gx (B, N, 6), gu (B, N, 2) (N axis dropped for 2-D
    inputs).  It differentiates the forward as it computes, the low-speed guard included: X and Y
    carry no derivative, vy, r and steer none for |vx| < 0.5 and vx none for |vx| < 0.3
    (include/mpcqp.h).  A caller whose stages share one (x, u) sums over the stage axis.
    ``out`` = (gx, gu): contiguous (B, N, 6) / (B, N, 2) tensors to write into."""
    return _linearise_vjp("linearise_vjp", veh, x, u, gAd, gBd, ggd, 6, out)


# ---- gradients with respect to a fleet's constants ----
def _fleet_of(fleet, kind, B, what):
    if not isinstance(fleet, kind):
        raise TypeError(f"{what} takes a {kind.__name__}: parameter gradients exist in fleet form only "
                        "(a uniform vehicle is a fleet of copies whose rows the caller sums)")
    if len(fleet) != B:
        raise ValueError(f"{what}: a fleet of {len(fleet)} vehicles was given a batch of {B}")
    return fleet._h


def _gk_out(out, B, nk, device):
    import torch
    if out is None:
        return torch.empty((B, nk), dtype=torch.float64, device=device)
    if tuple(out.shape) != (B, nk) or out.dtype != torch.float64 or not out.is_contiguous() or out.device != device:
        raise ValueError(f"out must be a contiguous float64 (B, {nk}) tensor on x's device")
    return out


def _linearise_pvjp(symbol, kind, fleet, x, u, gAd, gBd, ggd, nx, nk, out):
    import torch
    L = _bind()
    x, u, _ = _vjp_point(x, u, gAd, gBd, ggd, nx)
    B, N = x.shape[0], x.shape[1]
    h = _fleet_of(fleet, kind, B, symbol)
    gK = _gk_out(out, B, nk, x.device)
    _check(getattr(L, f"mpcqp_{symbol}_fleet_device")(
        h, B, N, _p(x), x.stride(0), x.stride(1), _p(u), u.stride(0), u.stride(1), _po(gAd), _po(gBd), _po(ggd),
        _p(gK), x.device.index or 0, _stream(torch, x.device)), symbol)
    return gK


def linearise_pvjp(fleet: Fleet, x, u, gAd, gBd, ggd, out=None):
    """d loss / d the fleet's constants through ``linearise`` (mpcqp_linearise_pvjp_fleet_device):
    x, u and the cotangents as ``linearise_vjp`` takes them -> gK (B, 13), summed over the N stages
    in stage order (deterministic: a repeated call returns the same bits; N <= 256), in the order of
    ``Fleet.constants()``.  ``Fleet.constants_vjp`` chains it to the constructor arguments.
    ``out``: a contiguous float64 (B, 13) tensor to write into."""
    return _linearise_pvjp("linearise_pvjp", Fleet, fleet, x, u, gAd, gBd, ggd, 6, 13, out)


def kin_linearise_pvjp(fleet: KinFleet, x, u, gAd, gBd, ggd, out=None):
    """The same through ``linearise_kinematics`` (mpcqp_kin_linearise_pvjp_fleet_device): gK (B, 3)
    in (l_f, l_r, dt)."""
    return _linearise_pvjp("kin_linearise_pvjp", KinFleet, fleet, x, u, gAd, gBd, ggd, 4, 3, out)


def _step_pvjp(symbol, kind, fleet, x, u, w, mode, nx, nk, out):
    import torch
    L = _bind()
    if x.dim() != 2 or u.dim() != 2 or x.shape[1] != nx or u.shape[1] != 2 or u.shape[0] != x.shape[0]:
        raise ValueError(f"x must be (B, {nx}) and u (B, 2)")
    if x.dtype != torch.float64 or u.dtype != torch.float64:
        raise ValueError("x and u must be float64")
    if x.stride(1) != 1 or u.stride(1) != 1:
        raise ValueError("the state / input axis must be contiguous")
    B = x.shape[0]
    if w is not None and (tuple(w.shape) != (B, nx) or w.dtype != torch.float64 or not w.is_contiguous()):
        raise ValueError(f"w must be a contiguous float64 (B, {nx}) tensor")
    if mode is not None:
        mode = _mode_in(mode, B, symbol)
    h = _fleet_of(fleet, kind, B, symbol)
    gK = _gk_out(out, B, nk, x.device)
    _check(getattr(L, f"mpcqp_{symbol}_fleet_device")(
        h, B, _p(x), x.stride(0), _p(u), u.stride(0), _po(w), _po(mode), _p(gK), x.device.index or 0,
        _stream(torch, x.device)), symbol)
    return gK


def euler_step_pvjp(fleet: Fleet, x, u, w, mode=None, out=None):
    """d loss / d the fleet's constants through the terminal step of ``incr_shift``
    (update_dynamics_model's guarded Euler step; mpcqp_euler_step_pvjp_fleet_device): x (B, 6),
    u (B, 2) with any batch stride (views into a taped solution), w (B, 6) the cotangent of the new
    state (None = zero), mode (B) int32 or None: a vehicle whose mode is not 0 gets a zero row
    -> gK (B, 13)."""
    return _step_pvjp("euler_step_pvjp", Fleet, fleet, x, u, w, mode, 6, 13, out)


def kin_update_pvjp(fleet: KinFleet, x, u, w, mode=None, out=None):
    """The same through ``kin_update``, the terminal step of the kinematic tails
    (mpcqp_kin_update_pvjp_fleet_device): x (B, 4), u (B, 2), w (B, 4) -> gK (B, 3)."""
    return _step_pvjp("kin_update_pvjp", KinFleet, fleet, x, u, w, mode, 4, 3, out)


class _Layout:
    """What IncrementalLayout and LTVLayout share: the marshalling of the weights, bounds and
    masks into mpcqp_<kind>_layout_create, the dimensions, the handle's lifetime, pattern()."""

    _kind = None  # "incr" / "ltv": the C ABI's prefix

    def __init__(self, N, Q, QN, R, bounds, maskA, maskB, device):
        L = _bind()
        Q = np.ascontiguousarray(np.asarray(sparse.csr_matrix(Q).todense(), np.float64))
        QN = np.ascontiguousarray(np.asarray(sparse.csr_matrix(QN).todense(), np.float64))
        R = np.ascontiguousarray(np.asarray(sparse.csr_matrix(R).todense(), np.float64))
        self.N, self.nx, self.nu = int(N), Q.shape[0], R.shape[0]
        arrs = [np.ascontiguousarray(np.asarray(a, np.float64).ravel()) for a in bounds]
        mA = np.ascontiguousarray(np.asarray(maskA, np.uint8))
        mB = np.ascontiguousarray(np.asarray(maskB, np.uint8))
        self._validate(Q, QN, R, arrs, mA, mB)
        h = C.c_void_p()
        _check(getattr(L, f"mpcqp_{self._kind}_layout_create")(
            self.N, self.nx, self.nu, _np_ptr(Q), _np_ptr(QN), _np_ptr(R), *(_np_ptr(a) for a in arrs), _np_ptr(mA),
            _np_ptr(mB), int(device), C.byref(h)), f"{self._kind}_layout_create")
        self._h = h.value
        # held: module globals may be gone at interpreter exit
        self._free = getattr(L, f"mpcqp_{self._kind}_layout_free")
        n, m, nP, nA = (C.c_int32() for _ in range(4))
        _check(getattr(L, f"mpcqp_{self._kind}_layout_dims")(self._h, C.byref(n), C.byref(m), C.byref(nP),
                                                             C.byref(nA)), "dims")
        self.n, self.m, self.nnzP, self.nnzA = n.value, m.value, nP.value, nA.value
        self.device = int(device)

    def _validate(self, Q, QN, R, arrs, mA, mB):
        pass

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._free(h)

    def pattern(self):
        """(P, A, l_template, u_template): scipy CSC templates (P upper triangle with its
        constant values; A with the constant entries and zeros at the stage entries) and
        the inequality-row bounds (clipped to +-1e30; equality rows 0)."""
        n, m = self.n, self.m
        Pp = np.zeros(n + 1, np.int32); Pi = np.zeros(self.nnzP, np.int32); Px = np.zeros(self.nnzP)
        Ap = np.zeros(n + 1, np.int32); Ai = np.zeros(self.nnzA, np.int32); At = np.zeros(self.nnzA)
        lt = np.zeros(m); ut = np.zeros(m)
        _check(getattr(lib(), f"mpcqp_{self._kind}_layout_pattern")(
            self._h, *(_np_ptr(a) for a in (Pp, Pi, Px, Ap, Ai, At, lt, ut))), "pattern")
        P = sparse.csc_matrix((Px, Pi, Pp), shape=(n, n))
        A = sparse.csc_matrix((At, Ai, Ap), shape=(m, n))
        return P, A, lt, ut

    def _empty_out(self, B, device):
        import torch
        kw = dict(dtype=torch.float64, device=device)
        return (torch.empty((B, self.nnzA), **kw), torch.empty((B, self.n), **kw),
                torch.empty((B, self.m), **kw), torch.empty((B, self.m), **kw))

    def _weights(self, weights):
        """weights = (Q, QN, R) of one call: float64 device tensors (nx,nx), (nx,nx), (nu,nu) shared
        by the batch, each None = the layout's own -> the three, checked and contiguous."""
        import torch
        if weights is None:
            return None, None, None
        out = []
        for t, w in zip(weights, (self.nx, self.nx, self.nu)):
            if t is not None and (tuple(t.shape) != (w, w) or t.dtype != torch.float64 or not t.is_cuda):
                raise ValueError(f"weights must be float64 device tensors of shapes ({self.nx}, {self.nx}), "
                                 f"({self.nx}, {self.nx}), ({self.nu}, {self.nu}) or None")
            out.append(None if t is None else t.contiguous())
        return out

    def _assemble_w(self, B, ins, bounds, weights, out, dev):
        """mpcqp_<kind>_assemble_w_device: `ins` the forward's five inputs, `bounds` (xlo, xhi) for
        the LTV layout and () for the incremental one -> (Ax, q, l, u, Px) with Px (nnzP,)."""
        import torch
        Ax, q, l, u = self._empty_out(B, dev) if out is None else out
        Px = torch.empty(self.nnzP, dtype=torch.float64, device=dev)
        keep = self._weights(weights)
        _check(getattr(lib(), f"mpcqp_{self._kind}_assemble_w_device")(
            self._h, B, *(_p(t) for t in ins), *(_po(t) for t in bounds), *(_po(t) for t in keep), _p(Ax), _p(q),
            _p(l), _p(u), _p(Px), _stream(torch, dev)), f"{self._kind}_assemble_w")
        return Ax, q, l, u, Px

    VJP_OUTPUTS = ("gAd", "gBd", "ggd", "gx0", "gXr", "gxlo", "gxhi", "gQ", "gQN", "gR")

    def assemble_vjp(self, gAx=None, gq=None, gl=None, gu=None, gPx=None, Xr=None, xlo=None, xhi=None,
                     weights=None, want=None, out=None):
        """The transpose of assemble() (mpcqp_<kind>_assemble_vjp_device; mpcqp.h has the formulas).
        Cotangents gAx (B,nnzA), gq (B,n), gl, gu (B,m), gPx (B,nnzP): contiguous float64 device
        tensors, None = zero (at least one given).  Xr, xlo, xhi, weights: the forward call's (Xr is
        read for gQ / gQN, xlo / xhi for gxlo / gxhi).  want: the outputs to form, of VJP_OUTPUTS
        (default: all the arguments allow); out: {name: tensor} to write into.  Returns a namespace
        with gAd (B,N,nx,nx), gBd (B,N,nx,nu), ggd (B,N,nx), gx0 (B,nxa), gXr (B,nx,N+1), gxlo, gxhi
        (B,N+1,nxa), gQ, gQN (B,nx,nx), gR (B,nu,nu) -- per instance, with respect to the stored
        weights -- and None for what was not wanted."""
        import torch
        from types import SimpleNamespace
        N, nx, nu, nxa = self.N, self.nx, self.nu, self.nxa
        cots = dict(gPx=(gPx, self.nnzP), gAx=(gAx, self.nnzA), gq=(gq, self.n), gl=(gl, self.m), gu=(gu, self.m))
        given = [t for t, _ in cots.values() if t is not None]
        if not given:
            raise ValueError("assemble_vjp: at least one cotangent must be given")
        B, dev = given[0].shape[0], given[0].device
        for k, (t, w) in cots.items():
            if t is not None and (tuple(t.shape) != (B, w) or t.dtype != torch.float64 or not t.is_contiguous()):
                raise ValueError(f"assemble_vjp: {k} must be a contiguous float64 tensor of shape ({B}, {w})")
        fwd = dict(Xr=(Xr, (B, nx, N + 1)), xlo=(xlo, (B, N + 1, nxa)), xhi=(xhi, (B, N + 1, nxa)))
        for k, (t, shape) in fwd.items():
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous()):
                raise ValueError(f"assemble_vjp: {k} must be a contiguous float64 tensor of shape {shape}")
        if self._kind != "ltv" and (xlo is not None or xhi is not None):
            raise ValueError("assemble_vjp: only the LTV layout takes per-stage bounds")
        shapes = dict(gAd=(B, N, nx, nx), gBd=(B, N, nx, nu), ggd=(B, N, nx), gx0=(B, nxa), gXr=(B, nx, N + 1),
                      gxlo=(B, N + 1, nxa), gxhi=(B, N + 1, nxa), gQ=(B, nx, nx), gQN=(B, nx, nx), gR=(B, nu, nu))
        if want is None:
            want = ["gAd", "gBd", "ggd", "gx0", "gXr"] + ["gxlo"] * (xlo is not None) + ["gxhi"] * (xhi is not None)
            if gPx is not None or (gq is not None and Xr is not None):
                want += ["gQ", "gQN", "gR"]
        bad = sorted(set(want) - set(shapes) | (set() if self._kind == "ltv" else set(want) & {"gxlo", "gxhi"}))
        if bad:
            raise ValueError(f"assemble_vjp: unknown output(s) {', '.join(bad)}")
        o = SimpleNamespace(**{k: None for k in shapes})
        for k in want:
            t = None if out is None else out.get(k)
            if t is None:
                t = torch.empty(shapes[k], dtype=torch.float64, device=dev)
            elif tuple(t.shape) != shapes[k] or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError(f"assemble_vjp: {k} must be a contiguous float64 tensor of shape {shapes[k]}")
            setattr(o, k, t)
        Q, QN, _ = self._weights(weights)
        ltv = self._kind == "ltv"
        args = [_po(gPx), _po(gAx), _po(gq), _po(gl), _po(gu), _po(Xr)] + ([_po(xlo), _po(xhi)] if ltv else [])
        args += [_po(Q), _po(QN)]
        args += [_po(getattr(o, k)) for k in self.VJP_OUTPUTS if ltv or k not in ("gxlo", "gxhi")]
        _check(getattr(lib(), f"mpcqp_{self._kind}_assemble_vjp_device")(self._h, B, *args, _stream(torch, dev)),
               f"{self._kind}_assemble_vjp")
        return o


class IncrementalLayout(_Layout):
    """The QP of mpc_increment (mpc_dynamics.py:281-389) for a batch sharing N, weights,
    bounds and the structural nonzeros of Ad / Bd (F1).  ``pattern()`` gives the CSC
    templates (P with its values, A), ``assemble()`` the per-instance values on the device."""

    _kind = "incr"

    def __init__(self, N, Q, QN, R, xmin_t, xmax_t, dumin, dumax, maskA=DYN_MASK_A, maskB=DYN_MASK_B, device=0):
        super().__init__(N, Q, QN, R, (xmin_t, xmax_t, dumin, dumax), maskA, maskB, device)
        self.nxa = self.nx + self.nu

    def assemble(self, Ad, Bd, gd, xt0, Xr, out=None, weights=None):
        """Ad (B,N,nx,nx), Bd (B,N,nx,nu), gd (B,N,nx), xt0 (B,nx+nu), Xr (B,nx,N+1), all
        contiguous float64 device tensors -> (Ax, q, l, u) in the layout's pattern order.
        weights = (Q, QN, R) device tensors (each None: the layout's own) assembles with the
        weights of this call (mpcqp_incr_assemble_w_device) and returns (Ax, q, l, u, Px), Px
        (nnzP,) being P's stored values from them, one copy for the batch."""
        import torch
        B = Ad.shape[0]
        for t in (Ad, Bd, gd, xt0, Xr):
            if not t.is_contiguous() or t.dtype != torch.float64:
                raise ValueError("assemble inputs must be contiguous float64 tensors")
        if weights is not None:
            return self._assemble_w(B, (Ad, Bd, gd, xt0, Xr), (), weights, out, Ad.device)
        if out is None:
            out = self._empty_out(B, Ad.device)
        Ax, q, l, u = out
        _check(lib().mpcqp_incr_assemble_device(self._h, B, _p(Ad), _p(Bd), _p(gd), _p(xt0), _p(Xr), _p(Ax), _p(q),
                                                _p(l), _p(u), _stream(torch, Ad.device)), "incr_assemble")
        return out


class AffineMap:
    """v = base[regime] + sum_t coef[:, t] * theta[idx[:, t]] over the concatenated (q | l | u)
    of an LTI layout -- the host description of mpcqp_affine (include/mpcqp.h), built by
    probing an assembler that is affine in theta: base[r] = build(0, r), and the terms of
    entry i from build(e_k, 0) for each parameter k.  `evaluate` applies it on the host
    (the CPU tests' check of the map against the builder); `LateralAssembler` uploads it."""

    def __init__(self, build, nparam, nregimes):
        outs0 = [np.concatenate(build(np.zeros(nparam), r)) for r in range(nregimes)]
        self.seglen = [len(v) for v in build(np.zeros(nparam), 0)]
        self.base = np.ascontiguousarray(np.stack(outs0))
        cols = []
        for k in range(nparam):
            e = np.zeros(nparam)
            e[k] = 1.0
            cols.append(np.concatenate(build(e, 0)) - outs0[0])
        Cm = np.stack(cols, axis=1) if cols else np.zeros((self.base.shape[1], 0))
        L = Cm.shape[0]
        nz = [np.flatnonzero(Cm[i]) for i in range(L)]
        self.T = max([len(z) for z in nz] + [0])
        self.idx = np.full((L, max(self.T, 1)), -1, np.int32)
        self.coef = np.zeros((L, max(self.T, 1)))
        for i, z in enumerate(nz):
            self.idx[i, :len(z)] = z
            self.coef[i, :len(z)] = Cm[i, z]
        # an entry that varies with theta has the same base in every regime (bounds change only
        # on constant rows), so one affine form per entry covers every regime
        var = np.array([len(z) > 0 for z in nz])
        if var.any() and not np.all(self.base[:, var] == self.base[:1, var]):
            raise ValueError("a theta-dependent entry changes with the regime: not an affine layout of this form")
        self.nparam, self.nregimes = nparam, nregimes

    def evaluate(self, theta, regime=None):
        """The device kernel's arithmetic (mpc_assembly.hip::k_affine) in numpy, per instance."""
        theta = np.atleast_2d(theta)
        B = theta.shape[0]
        reg = np.zeros(B, int) if regime is None else np.clip(np.asarray(regime), 0, self.nregimes - 1)
        out = np.empty((B, self.base.shape[1]))
        for b in range(B):
            bv = self.base[reg[b]]
            for i in range(out.shape[1]):
                v, anyt = 0.0, False
                for t in range(self.T):
                    k = self.idx[i, t]
                    if k >= 0:
                        term = self.coef[i, t] * theta[b, k]
                        v = v + term if anyt else term
                        anyt = True
                out[b, i] = bv[i] if not anyt else (bv[i] + v if bv[i] != 0.0 else v)
        s0, s1 = self.seglen[0], self.seglen[0] + self.seglen[1]
        return out[:, :s0], out[:, s0:s1], out[:, s1:]

    def vjp(self, gq, gl, gu):
        """The transpose of evaluate's linear part in the device kernel's order
        (mpc_assembly.hip::k_affine_vjp): gtheta[b, p] = sum of coef[i, t] * g[b, i] over the terms with
        idx[i, t] == p, entries ascending, then terms; g = (gq | gl | gu), each (B, seglen) or None."""
        segs = [None if g is None else np.atleast_2d(np.asarray(g, float)) for g in (gq, gl, gu)]
        B = next(g for g in segs if g is not None).shape[0]
        g = np.concatenate([np.zeros((B, w)) if s is None else s for s, w in zip(segs, self.seglen)], axis=1)
        out = np.zeros((B, self.nparam))
        first = np.ones(self.nparam, bool)
        for i in range(self.idx.shape[0]):
            for t in range(self.T):
                p = self.idx[i, t]
                if p >= 0:
                    term = self.coef[i, t] * g[:, i]
                    out[:, p] = term if first[p] else out[:, p] + term
                    first[p] = False
        return out


def lateral_builder(layout, N):
    """(build(theta, regime) -> (q, l, u), nparam, nregimes, (P, A)) of a lateral layout.
    vanilla (Control/MPC/mpc_kinematics.py:148-191 with the lateral Ad / Bd, cfg 2):
      theta = (x0 (4), Xr stage-major ((N+1) x 4)), one regime;
    slack (vehicle_lateral_mpc_slack_increment.py:48-115 and :201-229, cfg 1 / 3 / 4):
      theta = (x~0 (5), xr (4)), regime 0 (i <= 400 or i > 900) / 1 (400 < i <= 900, :163-167)."""
    from . import mpc
    if layout == "vanilla":
        def build(theta, regime):
            x0, Xr = theta[:4], theta[4:].reshape(N + 1, 4).T
            P, q, A, l, u = mpc.vanilla_qp(mpc.LATERAL_AD, mpc.LATERAL_BD, np.zeros(4), x0, Xr, mpc.VANILLA_Q,
                                           mpc.VANILLA_Q, mpc.VANILLA_R, N, mpc.VANILLA_XMIN, -mpc.VANILLA_XMIN,
                                           -mpc.VANILLA_UMAX, mpc.VANILLA_UMAX)
            return q, l, u
        nparam, nreg = 4 + 4 * (N + 1), 1
        P, _, A, _, _ = mpc.vanilla_qp(mpc.LATERAL_AD, mpc.LATERAL_BD, np.zeros(4), np.zeros(4), np.zeros((4, N + 1)),
                                       mpc.VANILLA_Q, mpc.VANILLA_Q, mpc.VANILLA_R, N, mpc.VANILLA_XMIN,
                                       -mpc.VANILLA_XMIN, -mpc.VANILLA_UMAX, mpc.VANILLA_UMAX)
    elif layout == "slack":
        def build(theta, regime):
            _, q, _, l, u = mpc.slack_qp(N, theta[:5], xr=theta[5:9], regime=regime)
            return q, l, u
        nparam, nreg = 9, 2
        P, _, A, _, _ = mpc.slack_qp(N, np.zeros(5))
    else:
        raise ValueError(layout)
    return build, nparam, nreg, (P, A)


class LateralAssembler:
    """F1 for the lateral layouts on the device: q, l, u of B instances from their parameters
    theta = (x0, xr) and bound regimes (mpcqp_affine_apply_device); P and A are the layout's
    own, the same for every instance (DeviceBatch.setup_solve with 1-D Px / Ax: the shared-
    matrix mode).  Replaces the reference's per-step rebuild of the whole QP in Python
    (vehicle_lateral_mpc_slack_increment.py:132-229, ~6.5 ms per step)."""

    def __init__(self, layout, N=20, device=0):
        L = _bind()
        build, nparam, nreg, (P, A) = lateral_builder(layout, N)
        self.map = AffineMap(build, nparam, nreg)
        self.P, self.A = P, A
        self.n, self.m = P.shape[0], A.shape[0]
        self.nparam, self.nregimes = nparam, nreg
        m = self.map
        seg = np.ascontiguousarray(np.array(m.seglen, np.int32))
        self._keep = (seg, m.base, np.ascontiguousarray(m.idx), np.ascontiguousarray(m.coef))
        h = C.c_void_p()
        _check(L.mpcqp_affine_create(len(m.seglen), _np_ptr(seg), m.nregimes, m.T, _np_ptr(m.base),
                                     _np_ptr(self._keep[2]), _np_ptr(self._keep[3]), int(device), C.byref(h)),
               "affine_create")
        self._h = h.value
        self._free = L.mpcqp_affine_free
        self.device = int(device)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._free(h)

    def matrices(self):
        """(Px, Ax): the layout's P (upper triangle) and A values in CSC order (host numpy)."""
        import scipy.sparse as sp
        P = sp.triu(sp.csc_matrix(self.P), format="csc")
        P.sort_indices()
        A = sp.csc_matrix(self.A)
        A.sort_indices()
        return P.data.copy(), A.data.copy()

    def assemble(self, theta, regime=None, out=None, stream=None):
        """theta (B, nparam) float64 and regime (B,) int32 device tensors -> (q, l, u) device
        tensors (into `out` when given)."""
        import torch
        L = _bind()
        B = theta.shape[0]
        if theta.dim() != 2 or theta.shape[1] < self.nparam or theta.stride(1) != 1:
            raise ValueError(f"theta must be (B, >= {self.nparam}) with a contiguous last axis")
        if regime is not None and (regime.dtype != torch.int32 or regime.shape[0] != B):
            raise ValueError("regime must be an int32 (B,) tensor")
        if out is None:
            kw = dict(dtype=torch.float64, device=theta.device)
            out = (torch.empty((B, self.n), **kw), torch.empty((B, self.m), **kw), torch.empty((B, self.m), **kw))
        st = stream if stream is not None else _stream(torch, theta.device)
        _check(L.mpcqp_affine_apply_device(self._h, B, _p(theta), theta.stride(0),
                                           None if regime is None else _p(regime), *(_p(t) for t in out), st),
               "affine_apply")
        return out

    def assemble_vjp(self, gq=None, gl=None, gu=None, regime=None, out=None, stream=None):
        """The transpose of assemble() (mpcqp_affine_vjp_device): cotangents gq (B, n), gl, gu
        (B, m), contiguous float64 device tensors, None = zero (at least one given) -> gtheta
        (B, nparam) (into `out` when given: (B, >= nparam) with a contiguous last axis).  The regime
        selects only the base, which has no derivative; it is accepted and ignored."""
        import torch
        L = _bind()
        given = [t for t in (gq, gl, gu) if t is not None]
        if not given:
            raise ValueError("assemble_vjp: at least one cotangent must be given")
        B, dev = given[0].shape[0], given[0].device
        for t, w in ((gq, self.n), (gl, self.m), (gu, self.m)):
            if t is not None and (tuple(t.shape) != (B, w) or t.dtype != torch.float64 or not t.is_contiguous()):
                raise ValueError(f"assemble_vjp: cotangents must be contiguous float64 ({B}, {self.n} / {self.m} / "
                                 f"{self.m}) tensors")
        if out is None:
            out = torch.empty((B, self.nparam), dtype=torch.float64, device=dev)
        elif out.dim() != 2 or out.shape[0] != B or out.shape[1] < self.nparam or out.stride(1) != 1 or \
                out.dtype != torch.float64:
            raise ValueError(f"assemble_vjp: out must be float64 (B, >= {self.nparam}) with a contiguous last axis")
        st = stream if stream is not None else _stream(torch, dev)
        _check(L.mpcqp_affine_vjp_device(self._h, B, _po(gq), _po(gl), _po(gu), _po(regime), _p(out), out.stride(0),
                                         st), "affine_vjp")
        return out


def reference_search(path_x, path_y, pred, dt):
    """reference_search (mpc_dynamics.py:44-90) per vehicle: pred (B, N+1, nxa) device tensor
    of predicted augmented states -> Xr (B, 6, N+1)."""
    import torch
    L = _bind()
    B, N1, nxa = pred.shape
    Xr = torch.empty((B, 6, N1), dtype=torch.float64, device=pred.device)
    _check(L.mpcqp_reference_search_device(B, N1 - 1, nxa, path_x.numel(), _p(path_x), _p(path_y), _p(pred),
                                           float(dt), _p(Xr), pred.device.index or 0, _stream(torch, pred.device)),
           "reference_search")
    return Xr


def _shift_in(t, shape, name):
    import torch
    if tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_cuda:
        raise ValueError(f"{name} must be a float64 device tensor of shape {shape}")
    return t.contiguous()


def incr_shift(layout, veh: Vehicle, sol, Ad, Bd, gd, xt):
    """Plant step and horizon shift of mpc_dynamics.main (mpcqp_incr_shift_device) as a function:
    sol (B, n), Ad (B, N, 6, 6), Bd (B, N, 6, 2), gd (B, N, 6) (stage 0 is read), xt (B, 8) ->
    (xt', pred', pdu') = new tensors (B, 8), (B, N+1, 8), (B, N+1, 2); nothing is written in place."""
    import torch
    B, N = sol.shape[0], layout.N
    sol = _shift_in(sol, (B, layout.n), "sol")
    Ad, Bd, gd = _shift_in(Ad, (B, N, 6, 6), "Ad"), _shift_in(Bd, (B, N, 6, 2), "Bd"), _shift_in(gd, (B, N, 6), "gd")
    xt1 = _shift_in(xt, (B, 8), "xt").clone()
    pred = torch.empty((B, N + 1, 8), dtype=torch.float64, device=sol.device)
    pdu = torch.empty((B, N + 1, 2), dtype=torch.float64, device=sol.device)
    fn, v = _entry("incr_shift", veh, B)
    _check(fn(layout._h, v, B, _p(sol), _p(Ad), _p(Bd), _p(gd), _p(xt1), _p(pred), _p(pdu),
              _stream(torch, sol.device)), "incr_shift")
    return xt1, pred, pdu


def _tail_vjp(name, symbol, layout, veh, B, head, cots, shapes, outputs, want, out, mode=None, prev=()):
    """What the tails' VJPs share: cotangent / output checks, the call (`head`: the entry point's
    arguments between B and the cotangents), and the pass-through cotangents of the previous horizon
    (`prev`: output name -> cotangent name, by `mode`)."""
    import torch
    from types import SimpleNamespace
    dev = head[0].device
    for k, t, shape in cots:
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError(f"{name}: {k} must be a contiguous float64 tensor of shape {shape}")
    want = list(outputs) if want is None else list(want)
    bad = sorted(set(want) - set(outputs))
    if bad:
        raise ValueError(f"{name}: unknown output(s) {', '.join(bad)}")
    o = SimpleNamespace(**{k: None for k in outputs})
    for k in want:
        t = None if out is None else out.get(k)
        if t is None:
            t = torch.empty(shapes[k], dtype=torch.float64, device=dev)
        elif tuple(t.shape) != shapes[k] or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"{name}: {k} must be a contiguous float64 tensor of shape {shapes[k]}")
        setattr(o, k, t)
    fn, v = _entry(name, veh, B)
    _check(fn(layout._h, v, B, *(_po(t) for t in head), *(_po(t) for _, t, _ in cots),
              *(_po(getattr(o, k)) for k in outputs), _stream(torch, dev)), name)
    given = {k: t for k, t, _ in cots}
    for k_out, k_cot in dict(prev).items():
        g = given[k_cot]
        if g is None:
            setattr(o, k_out, None)
        elif mode is None:
            setattr(o, k_out, torch.zeros_like(g))
        else:
            setattr(o, k_out, torch.where((mode == 1).view((-1,) + (1,) * (g.dim() - 1)), g, 0.0))
    return o


SHIFT_VJP_OUTPUTS = ("gsol", "gAd0", "gBd0", "ggd0", "gxt")


def incr_shift_vjp(layout, veh: Vehicle, sol, Ad, Bd, xt, gxt=None, gpred=None, gpdu=None, want=None, out=None):
    """The transpose of incr_shift (mpcqp_incr_shift_vjp_device; mpcqp.h has the formulas).  sol, Ad,
    Bd as the forward took them, xt the value from BEFORE the step; cotangents gxt (B, 8), gpred
    (B, N+1, 8), gpdu (B, N+1, 2) of the new xt, pred, pdu: contiguous float64 device tensors, None
    = zero.  want: the outputs to form, of SHIFT_VJP_OUTPUTS (default all); out: {name: tensor} to
    write into.  Returns a namespace with gsol (B, n), gAd0 (B, 6, 6), gBd0 (B, 6, 2), ggd0 (B, 6)
    -- the stage-0 model's, to be added into stage 0 -- and gxt (B, 8), None where not wanted."""
    B, N = sol.shape[0], layout.N
    sol = _shift_in(sol, (B, layout.n), "sol")
    Ad, Bd = _shift_in(Ad, (B, N, 6, 6), "Ad"), _shift_in(Bd, (B, N, 6, 2), "Bd")
    xt = _shift_in(xt, (B, 8), "xt")
    shapes = dict(gsol=(B, layout.n), gAd0=(B, 6, 6), gBd0=(B, 6, 2), ggd0=(B, 6), gxt=(B, 8))
    return _tail_vjp("incr_shift_vjp", "mpcqp_incr_shift_vjp_device", layout, veh, B, (sol, Ad, Bd, None, xt),
                     (("gxt", gxt, (B, 8)), ("gpred", gpred, (B, N + 1, 8)), ("gpdu", gpdu, (B, N + 1, 2))),
                     shapes, SHIFT_VJP_OUTPUTS, want, out)


def warm_shift(N, nxa, nu, x, y=None):
    """Shift an incremental-layout solution (x (B, n), y (B, m) device tensors) one stage
    forward for warm-starting the next step (mpcqp_incr_warm_shift_device)."""
    import torch
    L = _bind()
    xs = torch.empty_like(x)
    ys = None if y is None else torch.empty_like(y)
    _check(L.mpcqp_incr_warm_shift_device(x.shape[0], int(N), int(nxa), int(nu), _p(x),
                                          None if y is None else _p(y), _p(xs), None if y is None else _p(ys),
                                          x.device.index or 0, _stream(torch, x.device)), "incr_warm_shift")
    return xs, ys


class _ClosedLoop:
    """What the three closed loops share.  A subclass's __init__ builds its layout, calls
    ``_setup`` (solver, path, solve outputs), allocates its own state tensors and calls
    ``_start``; it states ``_linearise`` (the model's linearisation), ``_initial_horizon``,
    ``_reference``, ``_horizon`` (initial state, predicted states, predicted inputs) and ``_shift``.
    (LateralMPC, whose problem outlives the step, takes only ``step`` / ``_on_stream`` and the record
    from here and states its own ``_step``.)  A loop that records its trajectory allocates the
    record with ``_alloc_record`` and hands it out with ``trajectories``; DynamicMPC keeps none.

    Every kernel of a step runs on ``self.stream``, in order; a null (legacy default) torch
    stream would be passed as NULL, which the solver's C ABI reads as "the handle's own
    stream" -- unordered with torch's kernels."""

    def _setup(self, x0, u0, N, veh, device, layout, paths, settings, shift_warm):
        """x0 (B, layout.nx), u0 (B, 2); paths: name -> points, each kept as a device tensor
        under its name; settings: DeviceBatch's; shift_warm: start each solve from the last
        solution shifted one stage.  Returns x0, u0 as 2-D float64 arrays."""
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", device)
        self.veh, self.N, self.layout = veh, int(N), layout
        x0 = np.atleast_2d(np.asarray(x0, np.float64)); u0 = np.atleast_2d(np.asarray(u0, np.float64))
        if x0.shape[1] != layout.nx or u0.shape != (x0.shape[0], 2):
            raise ValueError(f"x0 must be (B, {layout.nx}) and u0 (B, 2)")
        self.B = x0.shape[0]
        if isinstance(veh, _FleetBase) and len(veh) != self.B:
            raise ValueError(f"a fleet of {len(veh)} vehicles was given a batch of {self.B}")
        P, A, _, _ = layout.pattern()
        settings.pop("verbose", None)
        self.shift_warm = bool(shift_warm)
        self.have_sol = False
        self.last = None
        self.solver = DeviceBatch(P, A, self.B, device=device, **settings)
        kw = dict(dtype=torch.float64, device=self.dev)
        ikw = dict(dtype=torch.int32, device=self.dev)
        self.Px = torch.from_numpy(np.tile(P.data, (self.B, 1))).to(**kw).contiguous()
        for name, p in paths.items():
            setattr(self, name, torch.as_tensor(np.ascontiguousarray(np.asarray(p, np.float64)), **kw).contiguous())
        if not all(getattr(self, name).numel() == self.path_x.numel() >= 2 for name in paths):
            raise ValueError(f"{', '.join(paths)} must have one length, at least 2")
        self.sol = torch.empty((self.B, layout.n), **kw)
        self.y = torch.empty((self.B, layout.m), **kw)
        self.status = torch.empty(self.B, **ikw)
        self.iters = torch.empty(self.B, **ikw)
        return x0, u0

    def _start(self):
        torch = self.torch
        self.stream = torch.cuda.Stream(self.dev)
        self._on_stream(self._initial_horizon)

    def _on_stream(self, fn):
        """fn() on self.stream, ordered after the caller's current stream; the caller's stream
        is ordered after it."""
        torch = self.torch
        caller = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(caller)
        with torch.cuda.stream(self.stream):
            out = fn()
        caller.wait_stream(self.stream)
        return out

    def _linearised_rollout(self):
        """Initial guess of the two incremental loops (mpc_dynamics.py:513-522,
        mpc_incre_kine_func.py:289-308): roll the linearised model forward with zero increments."""
        torch = self.torch
        nx = self.layout.nx
        pred = torch.empty((self.B, self.N + 1, nx + 2), dtype=torch.float64, device=self.dev)
        pred[:, 0] = self.xt
        xk = self.xt.clone()
        for i in range(self.N):
            Ad, Bd, gd = self._linearise(self.veh, xk[:, :nx].contiguous(), xk[:, nx:].contiguous(),
                                         self.dev.index or 0)
            x1 = torch.einsum("bij,bj->bi", Ad, xk[:, :nx]) + torch.einsum("bij,bj->bi", Bd, xk[:, nx:]) + gd
            xk = torch.cat([x1, xk[:, nx:] + self.pdu[:, i]], dim=1)
            pred[:, i + 1] = xk
        return pred

    def _alloc_record(self, traj_cap, width):
        """The trajectory record: traj (B, max(traj_cap, 1), width) zeros and traj_len (B,) zeros."""
        torch = self.torch
        self.traj_cap = int(traj_cap)
        self.traj = torch.zeros((self.B, max(self.traj_cap, 1), width), dtype=torch.float64, device=self.dev)
        self.traj_len = torch.zeros(self.B, dtype=torch.int32, device=self.dev)

    def step(self):
        """One receding-horizon step for every vehicle; returns (status, iters) device tensors.
        Asynchronous: ordered after the caller's current stream, and the caller's stream
        is ordered after the step."""
        return self._on_stream(self._step)

    def run(self, steps):
        """`steps` calls of step(); returns the last (status, iters)."""
        out = None
        for _ in range(int(steps)):
            out = self.step()
        return out

    def trajectories(self):
        """(traj, traj_len) as host arrays: traj (B, traj_cap, width) with the columns the class
        docstring names; traj_len[b] rows of traj[b] are filled."""
        return self.traj[:, :self.traj_cap].cpu().numpy(), self.traj_len.cpu().numpy()

    def _step(self):
        N = self.N
        Xr = self._reference()
        x0, xs, us = self._horizon()
        Ad, Bd, gd = self._linearise(self.veh, xs[:, :N], us[:, :N], self.dev.index or 0)
        Ax, q, l, u = self.layout.assemble(Ad, Bd, gd, x0, Xr)
        st = _stream(self.torch, self.dev)  # self.stream
        self.solver.setup(self.Px, Ax, q, l, u, stream=st)
        if self.shift_warm and self.have_sol:
            self.solver.warm_start(*warm_shift(N, self.layout.nxa, 2, self.sol, self.y), stream=st)
        self.solver.solve(self.sol, self.y, self.status, self.iters, stream=st)
        self.have_sol = True
        self._shift(_bind(), Ad, Bd, gd, Xr, st)
        self.last = dict(Ad=Ad, Bd=Bd, gd=gd, Xr=Xr, Ax=Ax, q=q, l=l, u=u)
        return self.status, self.iters


class DynamicMPC(_ClosedLoop):
    """B copies of mpc_dynamics.main's closed loop (:437-617), every step on the device.

    State per vehicle: x~ = (X, Y, yaw, vx, vy, r, steer, accel), the predicted
    horizon pred_x~ (N+1 stages) and pred_du.  ``step()`` = reference search ->
    linearisation of every predicted stage -> mpc_increment's QP -> batched OSQP
    solve (settings of :393: polish off, warm_start off) -> plant step and shift.

    ``warm_start=True`` (an extension; the reference solves every step cold) starts
    each solve from the previous step's solution shifted one stage (warm_shift)."""

    Q = np.diag([100.0, 100.0, 100.0, 50.0, 50.0, 50.0])          # :456-458
    QN = np.diag([1000.0, 1000.0, 1000.0, 500.0, 500.0, 500.0])
    R = np.diag([50.0, 50.0])
    DUMIN = np.array([-np.deg2rad(2.0), -0.5])                      # :461-464
    XMIN_T = np.array([-np.inf, -np.inf, -2 * np.pi, -100., -30., -0.5 * np.pi, -np.deg2rad(15), -3.])
    XMAX_T = np.array([np.inf, np.inf, 2 * np.pi, 100., 30., 0.5 * np.pi, np.deg2rad(15), 1.])
    _linearise = staticmethod(linearise)

    def __init__(self, x0, u0, path_x, path_y, N=30, veh: Vehicle | None = None, device=0, **solver_settings):
        layout = IncrementalLayout(int(N), self.Q, self.QN, self.R, self.XMIN_T, self.XMAX_T, self.DUMIN,
                                   -self.DUMIN, device=device)
        settings = {"polish": False, "warm_start": False, **solver_settings}   # mpc_dynamics.py:393
        x0, u0 = self._setup(x0, u0, N, veh or Vehicle(), device, layout, dict(path_x=path_x, path_y=path_y),
                             settings, settings.pop("warm_start"))
        kw = dict(dtype=self.torch.float64, device=self.dev)
        self.xt = self.torch.from_numpy(np.concatenate([x0, u0], axis=1)).to(**kw).contiguous()
        self.pdu = self.torch.zeros((self.B, self.N + 1, 2), **kw)
        self._start()

    def _initial_horizon(self):
        self.pred = self._linearised_rollout()

    def _reference(self):
        return reference_search(self.path_x, self.path_y, self.pred, self.veh.dt)

    def _horizon(self):
        return self.xt, self.pred[:, :, :6], self.pred[:, :, 6:]

    def _shift(self, L, Ad, Bd, gd, Xr, st):
        fn, v = _entry("incr_shift", self.veh, self.B)
        _check(fn(self.layout._h, v, self.B, _p(self.sol), _p(Ad), _p(Bd), _p(gd), _p(self.xt), _p(self.pred),
                  _p(self.pdu), st), "incr_shift")


# ------------------------------------------------------------ kinematic bicycle --
def linearise_kinematics(veh: KinVehicle, x, u, device=0):
    """Batched Vehicle_Kinematics.get_kinematics_model (vehicle_models.py:835-863).

    x: (B, N, 4) or (B, 4) float64 device tensor (X, Y, v, yaw), u: (B, N, 2) or (B, 2)
    (steer, accel), any strides with a contiguous last dimension -> Ad (B, N, 4, 4),
    Bd (B, N, 4, 2), gd (B, N, 4) (N axis dropped for 2-D inputs).  Inputs are not modified."""
    return _linearise("kin_linearise", veh, x, u, 4)


def linearise_kinematics_vjp(veh: KinVehicle, x, u, gAd, gBd, ggd):
    """The VJP of linearise_kinematics (mpcqp_kin_linearise_vjp_device): x, u as the forward took
    them (any strides with a contiguous last dimension -- a stage stride of 0 included), cotangents
    gAd (B, N, 4, 4), gBd (B, N, 4, 2), ggd (B, N, 4) contiguous float64 device tensors, None =
    zero -> dense gx (B, N, 4), gu (B, N, 2) (N axis dropped for 2-D inputs).  Only v, yaw and
    steer carry derivative; a caller whose stages share one (x, u) sums over the stage axis."""
    return _linearise_vjp("kin_linearise_vjp", veh, x, u, gAd, gBd, ggd, 4)


def reference_search_kin(path_x, path_y, path_yaw, set_speed, pred, dt):
    """reference_search of mpc_incre_kine_func.py (:42-81) per vehicle: pred (B, N+1, nxa)
    device tensor of predicted augmented states (speed in state 2), set_speed (B,)
    -> Xr (B, 4, N+1) with rows path x, path y, set_speed, path yaw."""
    import torch
    L = _bind()
    B, N1, nxa = pred.shape
    if path_y.numel() != path_x.numel() or path_yaw.numel() != path_x.numel() or set_speed.numel() != B:
        raise ValueError("path_x, path_y, path_yaw must have one length and set_speed B entries")
    for t in (path_x, path_y, path_yaw, set_speed, pred):
        if not t.is_contiguous() or t.dtype != torch.float64:
            raise ValueError("reference_search_kin inputs must be contiguous float64 tensors")
    Xr = torch.empty((B, 4, N1), dtype=torch.float64, device=pred.device)
    _check(L.mpcqp_kin_reference_search_device(B, N1 - 1, nxa, path_x.numel(), _p(path_x), _p(path_y), _p(path_yaw),
                                               _p(set_speed), _p(pred), float(dt), _p(Xr), pred.device.index or 0,
                                               _stream(torch, pred.device)), "kin_reference_search")
    return Xr


def _mode_in(mode, B, what):
    import torch
    if mode is not None and (tuple(mode.shape) != (B,) or mode.dtype != torch.int32 or not mode.is_cuda):
        raise ValueError(f"{what} must be an int32 device tensor of shape ({B},)")
    return None if mode is None else mode.contiguous()


def kin_shift(layout, veh: KinVehicle, sol, Ad, Bd, gd, Xr, xt, pred, pdu, finish_cnt=None, done=None):
    """The tail of simulate's loop (mpcqp_kin_shift_device, no trajectory record) as a function:
    sol (B, n), Ad (B, N, 4, 4), Bd (B, N, 4, 2), gd (B, N, 4) (stage 0 is read), Xr (B, 4, N+1), xt
    (B, 6), pred (B, N+1, 6), pdu (B, N+1, 2), finish_cnt / done int32 (B,) (None: zeros) ->
    (xt', pred', pdu', finish_cnt', done', mode), all new tensors; nothing is written in place.
    mode (B,) int32 is what kin_shift_vjp needs to know: 1 where done was already set (the vehicle
    was left untouched), 2 where this step set it (the stop rule: pred', pdu' are the unpacked
    solution, xt' = xt), 0 where the vehicle was stepped."""
    import torch
    B, N = sol.shape[0], layout.N
    sol = _shift_in(sol, (B, layout.n), "sol")
    Ad, Bd, gd = _shift_in(Ad, (B, N, 4, 4), "Ad"), _shift_in(Bd, (B, N, 4, 2), "Bd"), _shift_in(gd, (B, N, 4), "gd")
    Xr = _shift_in(Xr, (B, 4, N + 1), "Xr")
    xt1 = _shift_in(xt, (B, 6), "xt").clone()
    pred1 = _shift_in(pred, (B, N + 1, 6), "pred").clone()
    pdu1 = _shift_in(pdu, (B, N + 1, 2), "pdu").clone()
    ikw = dict(dtype=torch.int32, device=sol.device)
    cnt1 = torch.zeros(B, **ikw) if finish_cnt is None else finish_cnt.to(**ikw).clone()
    done0 = torch.zeros(B, **ikw) if done is None else done.to(**ikw).contiguous()
    done1 = done0.clone()
    fn, v = _entry("kin_shift", veh, B)
    _check(fn(layout._h, v, B, _p(sol), _p(Ad), _p(Bd), _p(gd), _p(Xr), _p(xt1), _p(pred1), _p(pdu1), _p(cnt1),
              _p(done1), None, 0, None, _stream(torch, sol.device)), "kin_shift")
    mode = torch.where(done0 != 0, 1, torch.where(done1 != 0, 2, 0)).to(torch.int32)
    return xt1, pred1, pdu1, cnt1, done1, mode


def kin_ltv_shift(layout, veh: KinVehicle, sol, status, Ad, Bd, gd, x, u, pred_x, pred_u):
    """The tail of mpc_kinematics_pred_matrix.main's loop (mpcqp_kin_ltv_shift_device, no trajectory
    record) as a function: sol (B, n), status (B,) int32 or None (all solved), Ad, Bd, gd as for
    kin_shift, x (B, 4), u (B, 2), pred_x (B, N+1, 4), pred_u (B, N+1, 2) -> (x', u', pred_x',
    pred_u', mode), all new tensors.  mode (B,) int32 = (status != 1): a skipped vehicle keeps x, u,
    pred_x, pred_u bit for bit."""
    import torch
    B, N = sol.shape[0], layout.N
    sol = _shift_in(sol, (B, layout.n), "sol")
    Ad, Bd, gd = _shift_in(Ad, (B, N, 4, 4), "Ad"), _shift_in(Bd, (B, N, 4, 2), "Bd"), _shift_in(gd, (B, N, 4), "gd")
    x1, u1 = _shift_in(x, (B, 4), "x").clone(), _shift_in(u, (B, 2), "u").clone()
    px1 = _shift_in(pred_x, (B, N + 1, 4), "pred_x").clone()
    pu1 = _shift_in(pred_u, (B, N + 1, 2), "pred_u").clone()
    ikw = dict(dtype=torch.int32, device=sol.device)
    if status is None:
        mode = torch.zeros(B, **ikw)
    else:
        status = _mode_in(status, B, "kin_ltv_shift: status")
        mode = (status != 1).to(torch.int32)
    skipped = torch.zeros(B, **ikw)
    fn, v = _entry("kin_ltv_shift", veh, B)
    _check(fn(layout._h, v, B, _p(sol), _po(status), _p(Ad), _p(Bd), _p(gd), _p(x1), _p(u1), _p(px1), _p(pu1),
              _p(skipped), None, None, 0, None, _stream(torch, sol.device)), "kin_ltv_shift")
    return x1, u1, px1, pu1, mode


KIN_LTV_SHIFT_VJP_OUTPUTS = ("gsol", "gAd0", "gBd0", "ggd0", "gx")


def kin_shift_vjp(layout, veh: KinVehicle, sol, Ad, Bd, xt, mode=None, gxt=None, gpred=None, gpdu=None, want=None,
                  out=None):
    """The transpose of kin_shift (mpcqp_kin_shift_vjp_device; mpcqp.h has the formulas and the
    modes).  sol, Ad, Bd as the forward took them, xt the value from BEFORE the step, mode kin_shift's
    (None: every vehicle stepped); cotangents gxt (B, 6), gpred (B, N+1, 6), gpdu (B, N+1, 2) of the
    new xt, pred, pdu: contiguous float64 device tensors, None = zero.  want / out as for
    incr_shift_vjp, over SHIFT_VJP_OUTPUTS.  Returns a namespace with gsol (B, n), gAd0 (B, 4, 4),
    gBd0 (B, 4, 2), ggd0 (B, 4), gxt (B, 6), and the cotangents of the PREVIOUS pred and pdu, which
    the kernel leaves to the caller: gpred_prev, gpdu_prev = the given cotangent where mode is 1,
    zero elsewhere (None for a None cotangent)."""
    B, N = sol.shape[0], layout.N
    sol = _shift_in(sol, (B, layout.n), "sol")
    Ad, Bd = _shift_in(Ad, (B, N, 4, 4), "Ad"), _shift_in(Bd, (B, N, 4, 2), "Bd")
    xt = _shift_in(xt, (B, 6), "xt")
    mode = _mode_in(mode, B, "kin_shift_vjp: mode")
    shapes = dict(gsol=(B, layout.n), gAd0=(B, 4, 4), gBd0=(B, 4, 2), ggd0=(B, 4), gxt=(B, 6))
    return _tail_vjp("kin_shift_vjp", "mpcqp_kin_shift_vjp_device", layout, veh, B, (sol, Ad, Bd, None, xt, mode),
                     (("gxt", gxt, (B, 6)), ("gpred", gpred, (B, N + 1, 6)), ("gpdu", gpdu, (B, N + 1, 2))),
                     shapes, SHIFT_VJP_OUTPUTS, want, out, mode, dict(gpred_prev="gpred", gpdu_prev="gpdu"))


def kin_ltv_shift_vjp(layout, veh: KinVehicle, sol, Ad, Bd, x, mode=None, gx=None, gu=None, gpred_x=None,
                      gpred_u=None, want=None, out=None):
    """The transpose of kin_ltv_shift (mpcqp_kin_ltv_shift_vjp_device).  x the state from BEFORE the
    step, mode kin_ltv_shift's; cotangents gx (B, 4), gu (B, 2), gpred_x (B, N+1, 4), gpred_u
    (B, N+1, 2) of the new x, u, pred_x, pred_u, None = zero.  Outputs KIN_LTV_SHIFT_VJP_OUTPUTS:
    gsol (B, n), gAd0 (B, 4, 4), gBd0 (B, 4, 2), ggd0 (B, 4), gx (B, 4); and the caller's part, the
    cotangents of the PREVIOUS u, pred_x, pred_u: gu_prev, gpred_x_prev, gpred_u_prev = the given
    cotangent where mode is 1, zero elsewhere (None for a None cotangent)."""
    B, N = sol.shape[0], layout.N
    sol = _shift_in(sol, (B, layout.n), "sol")
    Ad, Bd = _shift_in(Ad, (B, N, 4, 4), "Ad"), _shift_in(Bd, (B, N, 4, 2), "Bd")
    x = _shift_in(x, (B, 4), "x")
    mode = _mode_in(mode, B, "kin_ltv_shift_vjp: mode")
    shapes = dict(gsol=(B, layout.n), gAd0=(B, 4, 4), gBd0=(B, 4, 2), ggd0=(B, 4), gx=(B, 4))
    return _tail_vjp("kin_ltv_shift_vjp", "mpcqp_kin_ltv_shift_vjp_device", layout, veh, B, (sol, Ad, Bd, x, mode),
                     (("gx", gx, (B, 4)), ("gu", gu, (B, 2)), ("gpred_x", gpred_x, (B, N + 1, 4)),
                      ("gpred_u", gpred_u, (B, N + 1, 2))), shapes, KIN_LTV_SHIFT_VJP_OUTPUTS, want, out, mode,
                     dict(gu_prev="gu", gpred_x_prev="gpred_x", gpred_u_prev="gpred_u"))


class KinematicMPC(_ClosedLoop):
    """B copies of mpc_incre_kine_func.simulate(init_state, path_x, path_y, path_yaw)
    (:223-436), every step on the device.

    State per vehicle: x~ = (X, Y, v, yaw, steer, accel), the predicted horizon pred_x~
    (N+1 stages) and pred_du.  x0 is (B, 4), u0 (B, 2) (simulate's own u0 is (0, 0.01));
    set_speed is each vehicle's initial v (:279).  ``step()`` = reference search ->
    linearisation of every predicted stage -> mpc_increment's QP -> batched OSQP solve
    (settings of :180: polish off, warm_start off) -> trajectory record, stop rule, plant
    step and shift (mpcqp_kin_shift_device).

    Stop rule (:395-401): a vehicle within 0.5 of its first reference point counts up
    ``finish_cnt``; once the count exceeds 15 it is ``done`` and frozen -- its xt, pred,
    pdu, count and trajectory no longer change.

    ``trajectories()`` gives simulate's four lists as (traj (B, traj_cap, 4), traj_len):
    columns x, y, yaw and the step's first steer increment, one row per step a vehicle
    took while not done, rows beyond traj_cap dropped.  Row 0 is the initial state; its
    last column reproduces the reference, whose traj_steer starts with u0[1, 0] -- the
    initial ACCELERATION (:323), not a steer value.

    ``warm_start=True`` (an extension; the reference solves every step cold) starts
    each solve from the previous step's solution shifted one stage (warm_shift)."""

    _linearise = staticmethod(linearise_kinematics)

    def __init__(self, x0, u0, path_x, path_y, path_yaw, N=40, veh: KinVehicle | None = None, device=0, traj_cap=0,
                 **solver_settings):
        from . import mpc
        layout = IncrementalLayout(int(N), mpc.KIN_Q, mpc.KIN_QN, mpc.KIN_R, mpc.KIN_XMIN_T, mpc.KIN_XMAX_T,
                                   mpc.KIN_DUMIN, -mpc.KIN_DUMIN, maskA=mpc.KIN_MASK_A, maskB=mpc.KIN_MASK_B,
                                   device=device)
        settings = {"polish": False, "warm_start": False, **solver_settings}   # mpc_incre_kine_func.py:180
        x0, u0 = self._setup(x0, u0, N, veh or KinVehicle(), device, layout,
                             dict(path_x=path_x, path_y=path_y, path_yaw=path_yaw), settings,
                             settings.pop("warm_start"))
        torch = self.torch
        kw = dict(dtype=torch.float64, device=self.dev)
        ikw = dict(dtype=torch.int32, device=self.dev)
        self.xt = torch.from_numpy(np.concatenate([x0, u0], axis=1)).to(**kw).contiguous()
        self.set_speed = torch.from_numpy(np.ascontiguousarray(x0[:, 2])).to(**kw).contiguous()
        self.pdu = torch.zeros((self.B, self.N + 1, 2), **kw)             # del_u0 = 0 (:276, :293-296)
        self.finish_cnt = torch.zeros(self.B, **ikw)
        self.done = torch.zeros(self.B, **ikw)
        # the lists' first entries (:320-323): x0, y0, yaw0 and u0[1] (see the class docstring)
        self._alloc_record(traj_cap, 4)
        self.traj[:, 0] = torch.from_numpy(np.stack([x0[:, 0], x0[:, 1], x0[:, 3], u0[:, 1]], axis=1)).to(**kw)
        self.traj_len.fill_(1 if self.traj_cap > 0 else 0)
        self._start()

    def _initial_horizon(self):
        self.pred = self._linearised_rollout()

    def _reference(self):
        return reference_search_kin(self.path_x, self.path_y, self.path_yaw, self.set_speed, self.pred, self.veh.dt)

    def _horizon(self):
        return self.xt, self.pred[:, :, :4], self.pred[:, :, 4:]

    def _shift(self, L, Ad, Bd, gd, Xr, st):
        fn, v = _entry("kin_shift", self.veh, self.B)
        _check(fn(self.layout._h, v, self.B, _p(self.sol), _p(Ad), _p(Bd), _p(gd), _p(Xr), _p(self.xt), _p(self.pred),
                  _p(self.pdu), _p(self.finish_cnt), _p(self.done), _p(self.traj), self.traj_cap, _p(self.traj_len),
                  st), "kin_shift")

    def run(self, max_steps, check_every=16):
        """step() until every vehicle is done or max_steps steps were taken; returns the number
        of steps taken.  ``done`` is read back (one host synchronisation) only every
        `check_every` steps, so up to check_every - 1 steps may run after the last vehicle
        stopped.  A done vehicle is still solved with the rest of the batch: its state no
        longer moves, so its QP repeats from one step to the next and its solution is
        discarded."""
        check_every = max(int(check_every), 1)
        steps = 0
        while steps < max_steps:
            self.step()
            steps += 1
            if steps % check_every == 0 and bool(self.done.all().item()):
                break
        return steps


# ------------------------------------------------- LTV in the inputs themselves --
class LTVLayout(_Layout):
    """The QP of mpc__ (Control/MPC/mpc_kinematics_pred_matrix.py:268-352), mpc
    (mpc_dynamics.py:160-279) and mpc_ (mpc_kinematics.py:202-265) -- osqp_amd.mpc.ltv_qp --
    for a batch sharing N, weights, bounds and the structural nonzeros of Ad / Bd: variables
    (x_0..x_N, u_0..u_{N-1}), no u_prev augmentation.  ``pattern()`` gives the CSC templates,
    ``assemble()`` the per-instance values on the device (mpcqp_ltv_*)."""

    _kind = "ltv"

    def __init__(self, N, Q, QN, R, xmin, xmax, umin, umax, maskA, maskB, device=0):
        super().__init__(N, Q, QN, R, (xmin, xmax, umin, umax), maskA, maskB, device)
        self.nxa = self.nx  # no augmentation

    def _validate(self, Q, QN, R, arrs, mA, mB):
        if QN.shape != Q.shape or mA.shape != Q.shape or mB.shape != (self.nx, self.nu) or \
                [a.size for a in arrs] != [self.nx, self.nx, self.nu, self.nu]:
            raise ValueError("LTVLayout: Q, QN, maskA must be nx x nx, R nu x nu, maskB nx x nu, bounds nx / nu long")

    def assemble(self, Ad, Bd, gd, x0, Xr, xlo=None, xhi=None, out=None, weights=None):
        """Ad (B,N,nx,nx), Bd (B,N,nx,nu), gd (B,N,nx), x0 (B,nx), Xr (B,nx,N+1) and the optional
        per-stage state bounds xlo / xhi (B,N+1,nx), all contiguous float64 device tensors
        -> (Ax, q, l, u) in the layout's pattern order.  weights = (Q, QN, R) device tensors (each
        None: the layout's own) assembles with the weights of this call
        (mpcqp_ltv_assemble_w_device) and returns (Ax, q, l, u, Px), Px (nnzP,) being P's stored
        values from them, one copy for the batch."""
        import torch
        B, N, nx, nu = Ad.shape[0], self.N, self.nx, self.nu
        shapes = [(Ad, (B, N, nx, nx)), (Bd, (B, N, nx, nu)), (gd, (B, N, nx)), (x0, (B, nx)), (Xr, (B, nx, N + 1))]
        shapes += [(t, (B, N + 1, nx)) for t in (xlo, xhi) if t is not None]
        for t, shape in shapes:
            if tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float64:
                raise ValueError(f"assemble inputs must be contiguous float64 tensors; expected shape {shape}, "
                                 f"got {tuple(t.shape)}")
        if out is None:
            out = self._empty_out(B, Ad.device)
        Ax, q, l, u = out
        for t, w in ((Ax, self.nnzA), (q, self.n), (l, self.m), (u, self.m)):
            if tuple(t.shape) != (B, w) or not t.is_contiguous() or t.dtype != torch.float64:
                raise ValueError("assemble outputs must be contiguous float64 (B, nnzA / n / m / m) tensors")
        if weights is not None:
            return self._assemble_w(B, (Ad, Bd, gd, x0, Xr), (xlo, xhi), weights, out, Ad.device)
        _check(lib().mpcqp_ltv_assemble_device(self._h, B, _p(Ad), _p(Bd), _p(gd), _p(x0), _p(Xr),
                                               None if xlo is None else _p(xlo), None if xhi is None else _p(xhi),
                                               _p(Ax), _p(q), _p(l), _p(u), _stream(torch, Ad.device)),
               "ltv_assemble")
        return out


def rollout_kin(veh: KinVehicle, x0, u0, N):
    """Initial horizon of mpc_kinematics_pred_matrix.main (:405-419): x0 (B, 4), u0 (B, 2)
    contiguous float64 device tensors -> pred_x (B, N+1, 4) by update_kinematics_model under
    u0, pred_u (B, N+1, 2) = u0 in every stage (mpcqp_kin_rollout_device)."""
    import torch
    L = _bind()
    B = x0.shape[0]
    for t, w in ((x0, 4), (u0, 2)):
        if tuple(t.shape) != (B, w) or not t.is_contiguous() or t.dtype != torch.float64:
            raise ValueError("x0 must be (B, 4) and u0 (B, 2), contiguous float64")
    kw = dict(dtype=torch.float64, device=x0.device)
    pred_x = torch.empty((B, N + 1, 4), **kw); pred_u = torch.empty((B, N + 1, 2), **kw)
    fn, v = _entry("kin_rollout", veh, B)
    _check(fn(v, B, int(N), _p(x0), _p(u0), _p(pred_x), _p(pred_u), x0.device.index or 0,
              _stream(torch, x0.device)), "kin_rollout")
    return pred_x, pred_u


class KinematicLTVMPC(_ClosedLoop):
    """B copies of mpc_kinematics_pred_matrix.main's closed loop (:355-563), every step on
    the device.

    State per vehicle: x = (X, Y, v, yaw), u = (steer, accel), the predicted horizon pred_x
    (B, N+1, 4) and pred_u (B, N+1, 2).  x0 is (B, 4), u0 (B, 2) (main's own are (0, 0, 20, 0)
    and (0, 0.01)).  ``step()`` = reference search (set speed 10, path yaw 0, :40-82) ->
    linearisation of every predicted stage -> mpc__'s QP (LTVLayout) -> batched OSQP solve
    -> skip rule, trajectory record, plant step and shift (mpcqp_kin_ltv_shift_device).

    Skip rule (:480-484): a vehicle whose solve did not end `solved` (`solved inaccurate`
    included) keeps x, u, pred_x, pred_u and its trajectory as they are, and its ``skipped``
    count goes up; ``steps_taken`` counts the steps a vehicle executed.  A skipped vehicle of
    a cold-solving loop meets the same QP again and stays skipped, as in the reference.

    ``trajectories()`` gives (traj (B, traj_cap, 6), traj_len): columns x, y, v, yaw of the
    state a step started from and the steer, accel it applied (plt_states / plt_actions),
    one row per EXECUTED step, rows beyond traj_cap dropped.

    Settings are the reference's (:347, warm_start=True, polish off).  The reference builds a
    fresh solver object per step, so its warm_start never has anything to start from: every
    solve here is cold.  ``shift_warm=True`` (an extension) starts each solve from the previous
    step's solution shifted one stage (warm_shift)."""

    SET_SPEED = 10.0  # reference_search's x_ref[2] (:62)
    _linearise = staticmethod(linearise_kinematics)

    def __init__(self, x0, u0, path_x, path_y, N=100, veh: KinVehicle | None = None, device=0, traj_cap=0,
                 shift_warm=False, **solver_settings):
        from . import mpc
        layout = LTVLayout(int(N), mpc.KINLTV_Q, mpc.KINLTV_QN, mpc.KINLTV_R, mpc.KINLTV_XMIN, mpc.KINLTV_XMAX,
                           mpc.KINLTV_UMIN, mpc.KINLTV_UMAX, mpc.KIN_MASK_A, mpc.KIN_MASK_B, device=device)
        settings = {"polish": False, "warm_start": True, **solver_settings}   # mpc_kinematics_pred_matrix.py:347
        x0, u0 = self._setup(x0, u0, N, veh or KinVehicle(), device, layout, dict(path_x=path_x, path_y=path_y),
                             settings, shift_warm)
        torch = self.torch
        kw = dict(dtype=torch.float64, device=self.dev)
        ikw = dict(dtype=torch.int32, device=self.dev)
        self.path_yaw = torch.zeros_like(self.path_x)                      # x_ref[3] = deg2rad(0) (:63)
        self.set_speed = torch.full((self.B,), self.SET_SPEED, **kw)
        self.x = torch.from_numpy(x0).to(**kw).contiguous()
        self.u = torch.from_numpy(u0).to(**kw).contiguous()
        self.skipped = torch.zeros(self.B, **ikw)
        self.steps_taken = torch.zeros(self.B, **ikw)
        self._alloc_record(traj_cap, 6)
        self._start()

    def _initial_horizon(self):
        self.pred_x, self.pred_u = rollout_kin(self.veh, self.x, self.u, self.N)

    def _reference(self):
        return reference_search_kin(self.path_x, self.path_y, self.path_yaw, self.set_speed, self.pred_x,
                                    self.veh.dt)

    def _horizon(self):
        return self.x, self.pred_x, self.pred_u

    def _shift(self, L, Ad, Bd, gd, Xr, st):
        fn, v = _entry("kin_ltv_shift", self.veh, self.B)
        _check(fn(self.layout._h, v, self.B, _p(self.sol), _p(self.status), _p(Ad), _p(Bd), _p(gd), _p(self.x),
                  _p(self.u), _p(self.pred_x), _p(self.pred_u), _p(self.skipped), _p(self.steps_taken), _p(self.traj),
                  self.traj_cap, _p(self.traj_len), st), "kin_ltv_shift")


# ------------------------------------- a bank of paths, one selected per vehicle --
def reference_search_paths(paths_x, paths_y, paths_yaw, path_id, set_speed, pred, dt):
    """reference_search_kin over a bank of paths: paths_x, paths_y (npaths, npath) device tensors,
    paths_yaw the same or None (yaw 0 on every point), path_id (B,) int32 or None (path 0; an id
    outside the bank is clamped into it), set_speed (B,), pred (B, N+1, nxa)
    -> Xr (B, 4, N+1) (mpcqp_kin_reference_search_paths_device)."""
    import torch
    L = _bind()
    B, N1, nxa = pred.shape
    if paths_x.dim() != 2 or paths_y.shape != paths_x.shape or set_speed.numel() != B or \
            (paths_yaw is not None and paths_yaw.shape != paths_x.shape):
        raise ValueError("paths_x, paths_y, paths_yaw must be (npaths, npath) and set_speed have B entries")
    for t in (paths_x, paths_y, paths_yaw, set_speed, pred):
        if t is not None and (not t.is_contiguous() or t.dtype != torch.float64):
            raise ValueError("reference_search_paths inputs must be contiguous float64 tensors")
    if path_id is not None and (path_id.dtype != torch.int32 or tuple(path_id.shape) != (B,)
                                or not path_id.is_contiguous()):
        raise ValueError("path_id must be a contiguous int32 (B,) tensor")
    Xr = torch.empty((B, 4, N1), dtype=torch.float64, device=pred.device)
    _check(L.mpcqp_kin_reference_search_paths_device(
        B, N1 - 1, nxa, paths_x.shape[0], paths_x.shape[1], _p(paths_x), _p(paths_y),
        None if paths_yaw is None else _p(paths_yaw), None if path_id is None else _p(path_id), _p(set_speed),
        _p(pred), float(dt), _p(Xr), pred.device.index or 0, _stream(torch, pred.device)), "kin_reference_search_paths")
    return Xr


class LaneChangeMPC(_ClosedLoop):
    """B copies of mpc_increment_kinematics_pred_matrix.main's closed loop (:281-476, the double
    lane change), every step on the device.

    State per vehicle: x~ = (X, Y, v, yaw, steer, accel), the predicted horizon pred_x~ (N+1
    stages) and pred_du, as on KinematicMPC.  x0 is (B, 4), u0 (B, 2) (main's own are (0, 0, 20, 0)
    and (0, 0.01)).  path_x (npath,) is shared by the paths, paths_y is (npaths, npath): the
    script's scenario is paths_y = [0 x, 0 x + 4].  ``path_id`` (B,) says which path each vehicle's
    reference search runs on; it follows the step schedule of :380-391,
    path_id = paths_of[#{j : steps > switch_steps[j]}] (the script with sim_time = 1000: its
    switches are i > 50 and i > 150).  step0 (B,) int, default 0, is the schedule step each vehicle
    starts at, so one batch can hold vehicles at different points of the scenario.

    ``step()`` = reference search on the vehicle's path (set speed 10, yaw 0, :41-83) ->
    linearisation of every predicted stage -> mpc_increment's QP (IncrementalLayout with the
    mpc.LANE_* weights) -> batched OSQP solve (settings of :242: polish off, warm_start off) ->
    record, plant step, shift and schedule (mpcqp_lane_tail_device).  There is no skip rule: the
    script uses the solution whatever the solver's status (:248-252).

    ``trajectories()`` gives (traj (B, traj_cap, 6), traj_len): x, y, v, yaw, steer, accel of x~
    as each step started (plt_states / plt_actions: the input is the one held BEFORE the step),
    rows beyond traj_cap dropped.

    ``shift_warm=True`` (an extension; the script solves every step cold) starts each solve from
    the previous step's solution shifted one stage (warm_shift)."""

    SET_SPEED = 10.0  # reference_search's x_ref[2] (:63)
    _linearise = staticmethod(linearise_kinematics)

    def __init__(self, x0, u0, path_x, paths_y, N=40, switch_steps=LANE_SWITCH_STEPS, paths_of=LANE_PATHS_OF,
                 step0=None, veh: KinVehicle | None = None, device=0, traj_cap=0, shift_warm=False,
                 **solver_settings):
        from . import mpc
        self.switch_steps = np.ascontiguousarray(switch_steps, np.int32).reshape(-1)
        self.paths_of = np.ascontiguousarray(paths_of, np.int32).reshape(-1)
        path_x = np.asarray(path_x, np.float64).reshape(-1)
        paths_y = np.atleast_2d(np.asarray(paths_y, np.float64))
        if paths_y.shape[1] != path_x.size:
            raise ValueError("paths_y must be (npaths, npath) with npath = len(path_x)")
        if self.paths_of.size != self.switch_steps.size + 1 or self.switch_steps.size > 8:
            raise ValueError("paths_of must have one entry more than switch_steps (at most 8)")
        if self.paths_of.min() < 0 or self.paths_of.max() >= paths_y.shape[0]:
            raise ValueError(f"paths_of must lie in [0, {paths_y.shape[0]})")
        layout = IncrementalLayout(int(N), mpc.LANE_Q, mpc.LANE_QN, mpc.LANE_R, mpc.LANE_XMIN_T, mpc.LANE_XMAX_T,
                                   mpc.LANE_DUMIN, -mpc.LANE_DUMIN, maskA=mpc.KIN_MASK_A, maskB=mpc.KIN_MASK_B,
                                   device=device)
        settings = {"polish": False, "warm_start": False, **solver_settings}   # :242
        settings.pop("warm_start")  # every solve follows a fresh setup: cold unless shift_warm starts it
        x0, u0 = self._setup(x0, u0, N, veh or KinVehicle(), device, layout, dict(path_x=path_x), settings,
                             shift_warm)
        step0 = np.zeros(self.B, np.int32) if step0 is None else np.asarray(step0, np.int32).reshape(-1)
        if step0.shape != (self.B,):
            raise ValueError("step0 must be (B,)")
        torch = self.torch
        kw = dict(dtype=torch.float64, device=self.dev)
        ikw = dict(dtype=torch.int32, device=self.dev)
        self.paths_x = self.path_x.repeat(paths_y.shape[0], 1).contiguous()
        self.paths_y = torch.from_numpy(np.ascontiguousarray(paths_y)).to(**kw).contiguous()
        self.set_speed = torch.full((self.B,), self.SET_SPEED, **kw)
        self.xt = torch.from_numpy(np.concatenate([x0, u0], axis=1)).to(**kw).contiguous()
        self.pdu = torch.zeros((self.B, self.N + 1, 2), **kw)              # del_u0 = 0 (:331, :353-356)
        self.steps = torch.from_numpy(step0.copy()).to(**ikw)
        self.path_id = torch.from_numpy(mpc.lane_path_id(step0, self.switch_steps, self.paths_of)).to(**ikw)
        self._alloc_record(traj_cap, 6)
        self._start()

    def _initial_horizon(self):
        self.pred = self._linearised_rollout()                              # :350-368

    def _reference(self):
        return reference_search_paths(self.paths_x, self.paths_y, None, self.path_id, self.set_speed, self.pred,
                                      self.veh.dt)

    def _horizon(self):
        return self.xt, self.pred[:, :, :4], self.pred[:, :, 4:]

    def _shift(self, L, Ad, Bd, gd, Xr, st):
        fn, v = _entry("lane_tail", self.veh, self.B)
        _check(fn(self.layout._h, v, self.B, _p(self.sol), _p(Ad), _p(Bd), _p(gd), _p(self.xt), _p(self.pred),
                  _p(self.pdu), self.switch_steps.size, _np_ptr(self.switch_steps), _np_ptr(self.paths_of),
                  _p(self.steps), _p(self.path_id), _p(self.traj), self.traj_cap, _p(self.traj_len), st), "lane_tail")


class KinematicFrozenMPC(_ClosedLoop):
    """B copies of mpc_kinematics.main's closed loop (:268-461), every step on the device: the
    loop around the QP of `mpc` (:148-200) with ONE model per step, the linearisation at the
    current (x, u) -- u the control applied last -- on all N stages.

    State per vehicle: x = (X, Y, v, yaw), u = (steer, accel) and the predicted states pred_x
    (B, N+1, 4), which only the reference search reads.  x0 is (B, 4), u0 (B, 2) (main's own are
    (0, 0, 5, 30 deg) and (0, 0.01)).  pred_u0 (B, N+1, 2), default u0 in every stage, is the
    initial pred_u: the script draws it as u0 + noise (:318-323); the noise is the caller's.

    Initial horizon (:325-329, mpc.kinfrozen_rollout, on the host): pred_x stage 0 = x0, stage i
    = update_kinematics_model(stage i-1, pred_u0[i]) for 1 <= i <= N-1, stage N = 0.  The script
    rolls its own state forward while it does so (x0 IS x, :304), so the plant starts from
    pred_x stage N-1, not from x0; so does ``x`` here.

    ``step()`` = reference search on pred_x (set speed 10, yaw 0, :39-81) -> one linearisation
    (mpcqp_kin_linearise_device with stage stride 0) -> mpc's QP (LTVLayout with the
    mpc.KINFROZEN_* weights of the loop, :381-391) -> batched OSQP solve -> skip rule, unpack,
    record and plant step (mpcqp_kin_frozen_tail_device).  pred_x becomes the solution's states,
    stage 0 included, with no shift; the plant steps with the step's own linear model.

    Skip rule (:398-402): a vehicle whose solve did not end `solved` keeps x, u, pred_x and its
    trajectory, and ``skipped`` goes up.  It meets the same QP again, so it stays skipped for
    good, as in the reference.  ``steps_taken`` counts executed steps.

    ``trajectories()`` gives (traj (B, traj_cap, 6), traj_len): x, y, v, yaw a step started from
    and the steer, accel it applied, one row per executed step.

    Settings are the script's (:195, warm_start=True, polish off); a fresh problem is set up
    every step, so every solve is cold.  The loop has no shift, so no shift_warm is offered."""

    SET_SPEED = 10.0  # reference_search's x_ref[2] (:61)
    _linearise = staticmethod(linearise_kinematics)

    def __init__(self, x0, u0, path_x, path_y, N=100, pred_u0=None, veh: KinVehicle | None = None, device=0,
                 traj_cap=0, **solver_settings):
        from . import mpc
        if "shift_warm" in solver_settings:
            raise TypeError("KinematicFrozenMPC takes no shift_warm: the loop has no shift to warm-start from")
        if pred_u0 is not None:
            pred_u0 = np.asarray(pred_u0, np.float64)
            if pred_u0.shape != (np.atleast_2d(np.asarray(x0)).shape[0], int(N) + 1, 2):
                raise ValueError("pred_u0 must be (B, N+1, 2)")
        layout = LTVLayout(int(N), mpc.KINFROZEN_Q, mpc.KINFROZEN_QN, mpc.KINFROZEN_R, mpc.KINFROZEN_XMIN,
                           mpc.KINFROZEN_XMAX, mpc.KINFROZEN_UMIN, mpc.KINFROZEN_UMAX, mpc.KIN_MASK_A, mpc.KIN_MASK_B,
                           device=device)
        settings = {"polish": False, "warm_start": True, **solver_settings}   # mpc_kinematics.py:195
        x0, u0 = self._setup(x0, u0, N, veh or KinVehicle(), device, layout, dict(path_x=path_x, path_y=path_y),
                             settings, False)
        if pred_u0 is None:
            pred_u0 = np.repeat(u0[:, None], self.N + 1, 1)
        torch = self.torch
        kw = dict(dtype=torch.float64, device=self.dev)
        ikw = dict(dtype=torch.int32, device=self.dev)
        self.path_yaw = torch.zeros_like(self.path_x)                      # x_ref[3] = deg2rad(0) (:62)
        self.set_speed = torch.full((self.B,), self.SET_SPEED, **kw)
        v = self.veh
        if isinstance(v, _FleetBase):  # the host statement takes one wheelbase: vehicle by vehicle
            pred_x, x_start = mpc.per_vehicle(
                lambda l_f, l_r, dt, x, pu: mpc.kinfrozen_rollout(x, pu, self.N, l_f, l_r, dt),
                [(k.l_f, k.l_r, k.dt) for k in (v[b] for b in range(self.B))], x0, pred_u0)
        else:
            pred_x, x_start = mpc.kinfrozen_rollout(x0, pred_u0, self.N, v.l_f, v.l_r, v.dt)
        self.pred_x = torch.from_numpy(pred_x).to(**kw).contiguous()
        self.x = torch.from_numpy(x_start).to(**kw).contiguous()
        self.u = torch.from_numpy(u0).to(**kw).contiguous()
        self.skipped = torch.zeros(self.B, **ikw)
        self.steps_taken = torch.zeros(self.B, **ikw)
        self._alloc_record(traj_cap, 6)
        self._start()

    def _initial_horizon(self):
        pass  # rolled out on the host in __init__

    def _reference(self):
        return reference_search_kin(self.path_x, self.path_y, self.path_yaw, self.set_speed, self.pred_x,
                                    self.veh.dt)

    def _horizon(self):
        # the one model on every stage: (x, u) with stage stride 0
        return self.x, self.x[:, None, :].expand(self.B, self.N, 4), self.u[:, None, :].expand(self.B, self.N, 2)

    def _shift(self, L, Ad, Bd, gd, Xr, st):
        _check(L.mpcqp_kin_frozen_tail_device(self.layout._h, self.B, _p(self.sol), _p(self.status), _p(Ad), _p(Bd),
                                              _p(gd), _p(self.x), _p(self.u), _p(self.pred_x), _p(self.skipped),
                                              _p(self.steps_taken), _p(self.traj), self.traj_cap, _p(self.traj_len),
                                              st), "kin_frozen_tail")


# ------------------------------------------- the loop that keeps one problem alive --
class LateralMPC(_ClosedLoop):
    """B copies of vehicle_lateral_mpc_slack_increment.py's closed loop (:123-269), every step
    on the device: the one loop of the reference that keeps ONE osqp object alive -- setup()
    once with warm_start=True (:121), then per step update(q=, l=, u=) (:237) and a solve that
    starts from the previous step's iterates (:248).

    x0 is (B, 5): x~ = (beta, r, e_psi, e_y, u_prev), the script's own (0, 0, 5 deg, 3, 0); xr is
    (B, 4), default 0; step0 (B,) int, default 0, is the schedule step each vehicle starts at,
    so one batch can hold vehicles in different bound regimes (:158-172: switch_steps, regimes).
    ``theta`` (B, 9) = (x~, xr) is live: ``xt`` = theta[:, :5] is advanced by every step, and
    ``xr`` = theta[:, 5:] may be written between steps (the script's "dynamic reference", :125-129).

    Construction sets the problem up from assemble(theta, regime 0), as :87-121 set it up before
    the loop.  ``step()`` = LateralAssembler.assemble(theta, regime) -> DeviceBatch.update(q, l, u)
    -> DeviceBatch.solve -> mpcqp_lti_step_device (raise rule, record, plant step, schedule).
    The script's second update(l=, u=) with the new initial state (:267-269) is dropped: the
    next step's update overwrites it before any solve, and a bounds update only stores scaled
    data (no iterate, no rho changes with it).

    Failure rule (:252-253): a vehicle whose solve did not end `solved` (`solved inaccurate`
    included) is frozen where the script raises -- ``failed`` = 1, ``fail_step`` = its step
    counter, and xt, ``steps``, ``regime`` and its record never change again.  It is still
    solved with the rest of the batch; its solution is discarded.

    ``trajectories()`` gives (traj (B, traj_cap, 7), traj_len): plt_x_1..4 (the state a step
    started from), plt_u (the control after it), plt_del_u, plt_s, one row per executed step,
    rows beyond traj_cap dropped.

    Settings are the script's (warm_start=True, everything else OSQP's default) unless given."""

    def __init__(self, x0, xr=None, N=20, step0=None, device=0, traj_cap=0, switch_steps=SLACK_SWITCH_STEPS,
                 regimes=SLACK_REGIMES, **solver_settings):
        import torch
        from . import mpc
        self.torch = torch
        self.dev = torch.device("cuda", device)
        self.N = int(N)
        x0 = np.atleast_2d(np.asarray(x0, np.float64))
        self.B = B = x0.shape[0]
        xr = np.zeros((B, 4)) if xr is None else np.atleast_2d(np.asarray(xr, np.float64))
        step0 = np.zeros(B, np.int32) if step0 is None else np.asarray(step0, np.int32).reshape(-1)
        if x0.shape != (B, 5) or xr.shape != (B, 4) or step0.shape != (B,):
            raise ValueError("x0 must be (B, 5), xr (B, 4) and step0 (B,)")
        self.switch_steps = np.ascontiguousarray(switch_steps, np.int32).reshape(-1)
        self.regimes = np.ascontiguousarray(regimes, np.int32).reshape(-1)
        if self.regimes.size != self.switch_steps.size + 1 or self.switch_steps.size > 8:
            raise ValueError("regimes must have one entry more than switch_steps (at most 8)")
        self.asm = LateralAssembler("slack", N=self.N, device=device)
        if self.regimes.min() < 0 or self.regimes.max() >= self.asm.nregimes:
            raise ValueError(f"regimes must lie in [0, {self.asm.nregimes})")
        At, Bt = mpc.augment(mpc.LATERAL_AD, mpc.LATERAL_BD)
        self.At, self.Bt = np.ascontiguousarray(At), np.ascontiguousarray(Bt)
        self.nxa, self.nu = self.Bt.shape
        # x = (x~_0..x~_N, du_0..du_{N-1}, s_0..s_N): du_0 (:256) and the slack of e_y in s_0 (:259)
        self.du_off = (self.N + 1) * self.nxa
        self.slack_off = self.du_off + self.N * self.nu + 3
        settings = {"warm_start": True, **solver_settings}                 # :121
        settings.pop("verbose", None)
        self.solver = DeviceBatch(self.asm.P, self.asm.A, B, device=device, **settings)
        kw = dict(dtype=torch.float64, device=self.dev)
        ikw = dict(dtype=torch.int32, device=self.dev)
        self.Px, self.Ax = (torch.from_numpy(v).to(**kw).contiguous() for v in self.asm.matrices())
        self.theta = torch.from_numpy(np.concatenate([x0, xr], axis=1)).to(**kw).contiguous()
        self.xt, self.xr = self.theta[:, :5], self.theta[:, 5:]
        self.steps = torch.from_numpy(step0.copy()).to(**ikw)
        self.regime = torch.from_numpy(mpc.slack_regime(step0, self.switch_steps, self.regimes)).to(**ikw)
        self.failed = torch.zeros(B, **ikw)
        self.fail_step = torch.zeros(B, **ikw)
        self._alloc_record(traj_cap, self.nxa + self.nu + 1)
        n, m = self.asm.n, self.asm.m
        self.q, self.l, self.u = torch.empty((B, n), **kw), torch.empty((B, m), **kw), torch.empty((B, m), **kw)
        self.sol, self.y = torch.empty((B, n), **kw), torch.empty((B, m), **kw)
        self.status, self.iters = torch.empty(B, **ikw), torch.empty(B, **ikw)
        self.last = None
        self.stream = torch.cuda.Stream(self.dev)
        self._on_stream(self._setup_problem)

    def _setup_problem(self):
        st = _stream(self.torch, self.dev)  # self.stream
        self.asm.assemble(self.theta, None, out=(self.q, self.l, self.u), stream=st)
        self.solver.setup(self.Px, self.Ax, self.q, self.l, self.u, stream=st)

    def _step(self):
        st = _stream(self.torch, self.dev)  # self.stream
        self.asm.assemble(self.theta, self.regime, out=(self.q, self.l, self.u), stream=st)
        self.solver.update(self.q, self.l, self.u, stream=st)
        self.solver.solve(self.sol, self.y, self.status, self.iters, stream=st)
        self._tail(st)
        self.last = dict(q=self.q, l=self.l, u=self.u)
        return self.status, self.iters

    def _tail(self, st):
        """The loop's tail (:252-269) from sol / status: mpcqp_lti_step_device on stream `st`."""
        _check(_bind().mpcqp_lti_step_device(
            self.B, self.nxa, self.nu, _np_ptr(self.At), _np_ptr(self.Bt), self.asm.n, self.du_off, self.slack_off,
            _p(self.sol), _p(self.status), _p(self.theta), self.theta.stride(0), self.switch_steps.size,
            _np_ptr(self.switch_steps), _np_ptr(self.regimes), _p(self.steps), _p(self.regime), _p(self.failed),
            _p(self.fail_step), _p(self.traj), self.traj_cap, _p(self.traj_len), self.dev.index or 0, st), "lti_step")

    def run(self, nsim, strict=False, check_every=64):
        """`nsim` calls of step(); returns the last (status, iters).  With `strict`, ``failed`` is
        read back (one host synchronisation) every `check_every` steps and after the last one,
        and the script's ValueError('OSQP did not solve the problem!') is raised once any
        vehicle has failed -- up to check_every - 1 steps after it did."""
        check_every, nsim = max(int(check_every), 1), int(nsim)
        out = None
        for k in range(1, nsim + 1):
            out = self.step()
            if strict and (k % check_every == 0 or k == nsim) and bool(self.failed.any().item()):
                raise ValueError("OSQP did not solve the problem!")
        return out
