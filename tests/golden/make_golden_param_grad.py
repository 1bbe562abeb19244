"""Generate the parameter-gradient fixture from the reference's OWN code: the vehicle models with
each constructor argument perturbed up and down, for central differences.

Run where the reference checkout exists (see make_golden.py, whose stub machinery is imported
here: the path set-up and _save):
    MPLBACKEND=Agg python tests/golden/make_golden_param_grad.py

Only DATA is committed.  The cars are make_golden_fleet.py's three; the points are a subset of
linearise.npz / kin_linearise.npz, read from the committed fixtures: four outside the low-speed
guard and one in each of its two regions for each sign of vx (DYN_POINTS), so that the file stays
small with 2 x 2 x 9 perturbed models per car.

param_grad.npz (axis order of every perturbed output: car, argument, step (h, 2h), direction
(+, -), point):
  params (3, 9), kin_params (3, 3)   the constructor arguments, mpcqp_vehicle's / mpcqp_kin_vehicle's order
  steps (2,)                         the relative steps h and 2h: argument a moves by steps[k] * params[a]
  dyn_x, dyn_u, kin_x, kin_u         the points
  dyn_Ad, dyn_Bd, dyn_gd             Vehicle_Dynamics.get_dynamics_model      (vehicle_models.py:52-340)
  dyn_next                           update_dynamics_model                     (:343-477)
  kin_Ad, kin_Bd, kin_gd             Vehicle_Kinematics.get_kinematics_model  (:835-863)
  kin_next                           update_kinematics_model                   (:866-883)
"""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402
import make_golden_fleet as mf  # noqa: E402

STEPS = (1e-5, 2e-5)
DYN_ARGS = mf.FIELDS + ("dt",)
KIN_ARGS = ("l_f", "l_r", "dt")
# linearise.npz: vx 17.5, 5.7, 5.5, 5.8 | 0.1 (both regions), 0.4 (vy, r, steer only), -0.2, -0.45
DYN_POINTS = (0, 3, 12, 24, 40, 41, 42, 43)
KIN_POINTS = (0, 5, 11, 17, 23, 29, 35, 41)


def _perturbed(base, args):
    """[argument][step][direction] -> the keyword arguments with one of them moved"""
    out = []
    for a in args:
        out.append([[dict(base, **{a: base[a] * (1.0 + s * h)}) for s in (1.0, -1.0)] for h in STEPS])
    return out


def _dyn(kw, X, U):
    import vehicle_models
    veh = vehicle_models.Vehicle_Dynamics(turning_circle=mf.TURNING_CIRCLE, **kw)
    Ad, Bd, gd, nxt = [], [], [], []
    for x, u in zip(X, U):
        with contextlib.redirect_stdout(io.StringIO()):
            a, b, g = veh.get_dynamics_model(x.reshape(6, 1).copy(), u.reshape(2, 1).copy())
            n = veh.update_dynamics_model(x.reshape(6, 1).copy(), u.reshape(2, 1).copy())[0][:, 0]
        Ad.append(a); Bd.append(b); gd.append(g[:, 0]); nxt.append(n)
    return [np.stack(v) for v in (Ad, Bd, gd, nxt)]


def _kin(kw, X, U):
    import vehicle_models
    veh = vehicle_models.Vehicle_Kinematics(**kw)
    Ad, Bd, gd, nxt = [], [], [], []
    for x, u in zip(X, U):
        a, b, g = veh.get_kinematics_model(x.copy(), u.copy())
        Ad.append(a); Bd.append(b); gd.append(g[:, 0])
        nxt.append(np.asarray(veh.update_kinematics_model(x.copy(), u.copy()), float).reshape(4))
    return [np.stack(v) for v in (Ad, Bd, gd, nxt)]


def _sweep(model, bases, args, X, U):
    """the four outputs stacked as (car, argument, step, direction, point, ...)"""
    outs = [[[[model(kw, X, U) for kw in d] for d in s] for s in _perturbed(base, args)] for base in bases]
    return [np.array([[[[o[i] for o in d] for d in s] for s in a] for a in outs]) for i in range(4)]


def param_grad():
    d = np.load(os.path.join(mg.OUT, "linearise.npz"))
    Xd, Ud = d["x"][list(DYN_POINTS)], d["u"][list(DYN_POINTS)]
    d = np.load(os.path.join(mg.OUT, "kin_linearise.npz"))
    Xk, Uk = d["x"][list(KIN_POINTS)], d["u"][list(KIN_POINTS)]
    dyn_bases = [dict(mf.CARS[c], dt=mf.DT_DYN) for c in mf.CARS]
    kin_bases = [dict(l_f=mf.CARS[c]["l_f"], l_r=mf.CARS[c]["l_r"], dt=mf.DT_KIN) for c in mf.CARS]
    dAd, dBd, dgd, dn = _sweep(_dyn, dyn_bases, DYN_ARGS, Xd, Ud)
    kAd, kBd, kgd, kn = _sweep(_kin, kin_bases, KIN_ARGS, Xk, Uk)
    mg._save("param_grad.npz", dict(
        cars=np.array(list(mf.CARS)), steps=np.array(STEPS),
        params=np.array([[b[k] for k in DYN_ARGS] for b in dyn_bases], float),
        kin_params=np.array([[b[k] for k in KIN_ARGS] for b in kin_bases], float),
        dyn_x=Xd, dyn_u=Ud, kin_x=Xk, kin_u=Uk, dyn_Ad=dAd, dyn_Bd=dBd, dyn_gd=dgd, dyn_next=dn,
        kin_Ad=kAd, kin_Bd=kBd, kin_gd=kgd, kin_next=kn))


if __name__ == "__main__":
    mg._install_stub()
    param_grad()
