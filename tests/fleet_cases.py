"""The cars of the fleet tests (test helper): the three of tests/golden/make_golden_fleet.py, in an
order that does not put the default first, and the 130-vehicle sweep that crosses a 128-thread
block.  Constructor arguments only; dt is the model's (0.05 dynamic, 0.02 kinematic)."""
import numpy as np

from osqp_amd import mpc

TURNING_CIRCLE = 10.4
CARS = {
    "default": dict(m=1300, l_f=1.25, l_r=1.40, width=1.78, length=4.25, C_d=0.34, A_f=2.0, C_roll=0.015),
    "small": dict(m=950, l_f=1.05, l_r=1.25, width=1.60, length=3.60, C_d=0.30, A_f=1.8, C_roll=0.012),
    "van": dict(m=2400, l_f=1.55, l_r=1.75, width=2.00, length=5.40, C_d=0.40, A_f=3.2, C_roll=0.018),
}
ORDER = ("van", "default", "small")
DT_DYN, DT_KIN = 0.05, 0.02
B_SWEEP = 130


def params(car):
    """mpc.VehicleParams of a car."""
    return mpc.VehicleParams(turning_circle=TURNING_CIRCLE, dt=DT_DYN, **CARS[car])


def wheelbase(car):
    """(l_f, l_r, dt): what the kinematic host statements take."""
    return CARS[car]["l_f"], CARS[car]["l_r"], DT_KIN


def sweep():
    """B_SWEEP dynamic cars: m = 1000 + 5 b, l_f = 1.0 + 0.004 b, everything else default."""
    b = np.arange(B_SWEEP)
    return [dict(m=float(1000 + 5 * k), l_f=float(1.0 + 0.004 * k)) for k in b]


def vehicles(md, which):
    """Vehicle structs of mpc_device `md`: which = "cars" (ORDER) or "sweep"."""
    if which == "cars":
        return [md.Vehicle(dt=DT_DYN, **CARS[c]) for c in ORDER]
    return [md.Vehicle(dt=DT_DYN, **kw) for kw in sweep()]


def kin_vehicles(md, which):
    if which == "cars":
        return [md.KinVehicle(*wheelbase(c)) for c in ORDER]
    return [md.KinVehicle(l_f=kw["l_f"], dt=DT_KIN) for kw in sweep()]
