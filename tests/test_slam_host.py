"""Host side of loop closure in the frame loop (include/lo_odometry.h): the defaults, the two new structs' layout
against their ctypes mirrors (the small C program of tests/test_header_abi.py, for these structs), and the null-handle
returns.  No GPU call is made.
"""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

from lidar_odometry_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.dirname(_lib.LIB_PATH)

STRUCTS = {"lo_loop_config": _lib.LoLoopConfig, "lo_loop_event": _lib.LoLoopEvent}
NESTED = {"lo_loop_config": {"iris": ("similarity_threshold", "min_keyframe_gap", "max_search_distance")}}


def test_loop_config_defaults_are_the_reference_s():
    """ConfigUtils.h:117-134: similarity 0.3f, keyframe gap 50 (both of its uses), search distance 10 m, PGO noises
    0.5 / 0.5 / 1.0 / 1.0; the inlier gate 0.3f of Estimator.cpp:1015."""
    c = _lib.LoLoopConfig()
    C.memset(C.byref(c), 0xFF, C.sizeof(c))
    _lib.lib().lo_loop_config_default(C.byref(c))
    assert c.iris.similarity_threshold == C.c_float(0.3).value
    assert c.iris.min_keyframe_gap == 50
    assert c.iris.max_search_distance == 10.0
    assert c.cooldown_keyframes == 50
    assert c.min_inlier_ratio == C.c_float(0.3).value
    assert (c.odom_trans_noise, c.odom_rot_noise, c.loop_trans_noise, c.loop_rot_noise) == (0.5, 0.5, 1.0, 1.0)
    assert c.max_keyframes >= 1 and c.max_points >= 1
    _lib.lib().lo_loop_config_default(None)                        # a null pointer is ignored


def test_python_loop_config_round_trip():
    from lidar_odometry_amd.odometry import LoopConfig
    c = LoopConfig(similarity_threshold=0.4, min_keyframe_gap=6, cooldown_keyframes=7, max_keyframes=64,
                   max_points=12345).to_c()
    assert c.iris.similarity_threshold == C.c_float(0.4).value
    assert (c.iris.min_keyframe_gap, c.cooldown_keyframes, c.max_keyframes, c.max_points) == (6, 7, 64, 12345)
    d = LoopConfig().to_c()
    e = _lib.LoLoopConfig()
    _lib.lib().lo_loop_config_default(C.byref(e))
    assert bytes(d) == bytes(e)


def _source():
    lines = ['#include "lo_odometry.h"', "#include <stdio.h>", "#include <stddef.h>", "", "int main(void) {",
             '    printf("{\\"ok\\": 1");']
    for name, cls in STRUCTS.items():
        lines.append(f'    printf(", \\"{name}\\": {{\\"size\\": %d", (int)sizeof({name}));')
        for fname, _ in cls._fields_:
            lines.append(f'    printf(", \\"{fname}\\": %d", (int)offsetof({name}, {fname}));')
            for sub in NESTED.get(name, {}).get(fname, ()):
                lines.append(f'    printf(", \\"{fname}.{sub}\\": %d", (int)offsetof({name}, {fname}.{sub}));')
        lines.append('    printf("}");')
    lines += ['    printf("}\\n");', "    return 0;", "}"]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_new_structs_match_their_ctypes_mirrors(tmp_path, lang):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.skip("no host compiler")
    src = tmp_path / ("slam_abi.c" if lang == "c" else "slam_abi.cpp")
    src.write_text(_source())
    exe = tmp_path / "slam_abi"
    std = ["-std=c99"] if lang == "c" else ["-std=c++17"]
    p = subprocess.run([cc, *std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    for name, cls in STRUCTS.items():
        want = {"size": C.sizeof(cls)}
        for fname, ftype in cls._fields_:
            off = getattr(cls, fname).offset
            want[fname] = off
            for sub in NESTED.get(name, {}).get(fname, ()):
                want[f"{fname}.{sub}"] = off + getattr(ftype, sub).offset
        assert got[name] == want, (name, got[name], want)


def test_null_handles_are_argument_errors():
    L = _lib.lib()
    cfg = _lib.LoLoopConfig()
    L.lo_loop_config_default(C.byref(cfg))
    ev = _lib.LoLoopEvent()
    n = C.c_size_t(7)
    assert L.lo_odom_enable_loop_closure(None, C.byref(cfg)) == _lib.LO_ERR_ARG
    assert L.lo_odom_last_loop(None, C.byref(ev)) == _lib.LO_ERR_ARG
    assert L.lo_odom_loop_count(None) == 0
    assert L.lo_odom_keyframe_poses(None, None, None, 0) == 0
    assert L.lo_odom_build_map(None, 0.5, C.byref(n)) == _lib.LO_ERR_ARG
    assert L.lo_odom_map_points(None, None, 0) == _lib.LO_ERR_ARG
    assert L.lo_odom_save_map_ply(None, b"unused.ply", 0.5) == _lib.LO_ERR_ARG
    kid, p = C.c_int64(0), C.c_void_p(0)
    assert L.lo_gmap_keyframe_points(None, 0, C.byref(kid), C.byref(p), C.byref(n)) == _lib.LO_ERR_ARG
    T = (C.c_float * 12)()
    inl = C.c_float(0.0)
    assert L.lo_icp_optimize_loop_dev(None, None, 0, T, None, 0, T, T, C.byref(inl), None, None) == _lib.LO_ERR_ARG
    assert L.lo_loop_reruns(None) == -1
