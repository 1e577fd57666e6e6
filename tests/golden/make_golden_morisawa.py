#!/usr/bin/env python3
"""Makes tests/golden/morisawa_shortwalk_datref.npz from the reference's two golden files of its Morisawa-2007 short walk:

    python tests/golden/make_golden_morisawa.py <reference tree>

reads <reference tree>/tests/TestMorisawa2007ShortWalk{32,64}TestFGPI.datref.cmake and keeps, as data, the columns the analytic
walk produces: time, CoM x y z, dCoM x y, ZMP x y, and x y z theta omega omega2 of both feet.  The 32-bit file has the 38 columns
tests/TestObject.cpp:344-385 writes; the 64-bit file has the older 26-column layout (no foot velocities and accelerations).
Both maps are recorded in the file, with the step sequence of tests/TestMorisawa2007.cpp:117 and the parameters of
tests/CommonTools.cpp:57-67.  The start CoM is not in the reference's data (it comes from its HRP-2 model); the test fits it."""
import os
import sys

import numpy as np

NAMES = ("time", "com_x", "com_y", "com_z", "dcom_x", "dcom_y", "zmp_x", "zmp_y",
         "left_x", "left_y", "left_z", "left_theta", "left_omega", "left_omega2",
         "right_x", "right_y", "right_z", "right_theta", "right_omega", "right_omega2")
# 0-based column of each name
MAP38 = (0, 1, 2, 3, 5, 6, 8, 9, 10, 11, 12, 19, 20, 21, 22, 23, 24, 31, 32, 33)
MAP26 = (0, 1, 2, 3, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21)
# ":stepseq" of AnalyticalShortStraightWalking (TestMorisawa2007.cpp:117): sx, sy, theta (degrees)
STEPS = ((0.0, -0.105, 0.0), (0.2, 0.19, 0.0), (0.2, -0.19, 0.0), (0.2, 0.19, 0.0), (0.2, -0.19, 0.0), (0.2, 0.19, 0.0),
         (0.0, -0.19, 0.0))
# CommonInitialization (CommonTools.cpp:57-67): sampling period, single and double support time, step height, omega
MODEL = dict(T=0.005, t_single=0.78, t_double=0.02, step_height=0.07, omega=0.0)


def main():
    ref = sys.argv[1]
    out = {}
    for bits, cmap in ((32, MAP38), (64, MAP26)):
        a = np.loadtxt(os.path.join(ref, "tests", "TestMorisawa2007ShortWalk%dTestFGPI.datref.cmake" % bits))
        assert a.shape[1] == (38 if bits == 32 else 26), a.shape
        out["data%d" % bits] = np.ascontiguousarray(a[:, list(cmap)])
        out["map%d" % bits] = np.array(cmap, dtype=np.int32)
    out["names"] = np.array(NAMES)
    out["steps"] = np.array(STEPS, dtype=np.float64)
    out["model"] = np.array([MODEL[k] for k in ("T", "t_single", "t_double", "step_height", "omega")], dtype=np.float64)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "morisawa_shortwalk_datref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", out["data32"].shape, out["data64"].shape)


if __name__ == "__main__":
    main()
