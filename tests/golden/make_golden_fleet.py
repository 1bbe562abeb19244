"""Generate the fleet fixtures from the reference's OWN code: the vehicle models for cars other
than the one every other fixture was captured with (m 1300, l_f 1.25, l_r 1.40).

Run where the reference checkout exists (see make_golden.py, whose stub machinery is imported
here: the path set-up and _save):
    MPLBACKEND=Agg python tests/golden/make_golden_fleet.py [linearise_fleet kin_linearise_fleet update_fleet]

Only DATA is committed.  The points are those of linearise.npz and kin_linearise.npz, read from
the committed fixtures, so the three cars are compared on the points the default car already is.

Fixtures (axis 0 of every output is the car, in the order of `cars`):
  linearise_fleet.npz      Vehicle_Dynamics.get_dynamics_model (vehicle_models.py:52-340) at
                           linearise.npz's 48 (x, u) for the cars of CARS, with their nine
                           constructor arguments (`params`, in mpcqp_vehicle's order) and
                           turning_circle
  kin_linearise_fleet.npz  Vehicle_Kinematics.get_kinematics_model (:835-863) at kin_linearise.npz's
                           48 (x, u) for the three wheelbases (`params`: l_f, l_r, dt)
  update_fleet.npz         update_dynamics_model (:343-477) and update_kinematics_model (:866-883)
                           at the same points: the terminal steps of the loops' horizon shifts
"""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402

TURNING_CIRCLE = 10.4
DT_DYN, DT_KIN = 0.05, 0.02
FIELDS = ("m", "l_f", "l_r", "width", "length", "C_d", "A_f", "C_roll")
CARS = {
    "default": dict(m=1300, l_f=1.25, l_r=1.40, width=1.78, length=4.25, C_d=0.34, A_f=2.0, C_roll=0.015),
    "small": dict(m=950, l_f=1.05, l_r=1.25, width=1.60, length=3.60, C_d=0.30, A_f=1.8, C_roll=0.012),
    "van": dict(m=2400, l_f=1.55, l_r=1.75, width=2.00, length=5.40, C_d=0.40, A_f=3.2, C_roll=0.018),
}


def _points(name):
    d = np.load(os.path.join(mg.OUT, name))
    return d["x"], d["u"]


def _dynamic(car):
    import vehicle_models
    return vehicle_models.Vehicle_Dynamics(turning_circle=TURNING_CIRCLE, dt=DT_DYN, **CARS[car])


def _kinematic(car):
    import vehicle_models
    return vehicle_models.Vehicle_Kinematics(l_f=CARS[car]["l_f"], l_r=CARS[car]["l_r"], dt=DT_KIN)


def _names():
    return np.array(list(CARS))


def linearise_fleet():
    X, U = _points("linearise.npz")
    Ad, Bd, gd = [], [], []
    for car in CARS:
        veh = _dynamic(car)
        out = []
        for x, u in zip(X, U):
            with contextlib.redirect_stdout(io.StringIO()):
                out.append(veh.get_dynamics_model(x.reshape(6, 1).copy(), u.reshape(2, 1).copy()))
        Ad.append(np.stack([o[0] for o in out])); Bd.append(np.stack([o[1] for o in out]))
        gd.append(np.stack([o[2][:, 0] for o in out]))
    params = np.array([[CARS[c][k] for k in FIELDS] + [DT_DYN] for c in CARS], float)
    mg._save("linearise_fleet.npz", dict(cars=_names(), params=params, turning_circle=np.array(TURNING_CIRCLE), x=X,
                                         u=U, Ad=np.stack(Ad), Bd=np.stack(Bd), gd=np.stack(gd)))


def kin_linearise_fleet():
    X, U = _points("kin_linearise.npz")
    Ad, Bd, gd = [], [], []
    for car in CARS:
        veh = _kinematic(car)
        out = [veh.get_kinematics_model(x.copy(), u.copy()) for x, u in zip(X, U)]
        Ad.append(np.stack([o[0] for o in out])); Bd.append(np.stack([o[1] for o in out]))
        gd.append(np.stack([o[2][:, 0] for o in out]))
    params = np.array([[CARS[c]["l_f"], CARS[c]["l_r"], DT_KIN] for c in CARS], float)
    mg._save("kin_linearise_fleet.npz", dict(cars=_names(), params=params, x=X, u=U, Ad=np.stack(Ad),
                                             Bd=np.stack(Bd), gd=np.stack(gd)))


def update_fleet():
    Xd, Ud = _points("linearise.npz")
    Xk, Uk = _points("kin_linearise.npz")
    dyn, kin = [], []
    for car in CARS:
        veh = _dynamic(car)
        with contextlib.redirect_stdout(io.StringIO()):
            dyn.append(np.stack([veh.update_dynamics_model(x.reshape(6, 1).copy(), u.reshape(2, 1).copy())[0][:, 0]
                                 for x, u in zip(Xd, Ud)]))
        veh = _kinematic(car)
        kin.append(np.stack([np.asarray(veh.update_kinematics_model(x.copy(), u.copy()), float).reshape(4)
                             for x, u in zip(Xk, Uk)]))
    mg._save("update_fleet.npz", dict(cars=_names(), dyn_x=Xd, dyn_u=Ud, dyn_next=np.stack(dyn), kin_x=Xk, kin_u=Uk,
                                      kin_next=np.stack(kin)))


if __name__ == "__main__":
    mg._install_stub()
    which = set(sys.argv[1:])
    for f in (linearise_fleet, kin_linearise_fleet, update_fleet):
        if not which or f.__name__ in which:
            f()
