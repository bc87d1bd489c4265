"""Restatements of what an EndToEndKartAgent (the reference's AI/EndToEndKartAgent.cs, "E2E") computes differently from a
HierarchicalKartAgent, in float32 numpy, from hk_agent_state records and the track table alone.  The CPU oracle cannot model
E2E agents, so the E2E rows of libhk are held to these (tests/test_e2e_cpu.py, tests/test_e2e_gpu.py).

  observe_e2e     CollectObservations E2E:279-376: own block and section horizon (the team / opponent blocks and the nine rays are
                  HKA's and come from the oracle's row of the same kart)
  academy_e2e     OnActionReceived E2E:385-415: the base KartAgent rewards (aimed at the planned lane box when there is one), then the
                  same three rewards again aimed at the next Trigger

The kart's forward vector is sin / cos of its yaw through the library's own fp32 sincos (include/hk_detmath.h hk_sincosf), compiled
here into a small host library so that the restatement rounds exactly as the kernels do."""
import ctypes as C
import os
import subprocess
import tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SHIM = None
f32 = np.float32

_SHIM_SRC = r'''
#include "hk_detmath.h"
void e2e_sincosf(const float* x, float* s, float* c, int n) { for (int i = 0; i < n; i++) hk_sincosf(x[i], &s[i], &c[i]); }
'''


def _shim():
    """built once under build/ (beside the other build products) and rebuilt when include/hk_detmath.h is newer; written to a temporary
    name and renamed, so that concurrent test processes never load a half-written library"""
    global _SHIM
    if _SHIM is None:
        d = os.path.join(ROOT, "build", "test_shims")
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, "e2e_sincosf.so")
        hdr = os.path.join(ROOT, "include", "hk_detmath.h")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(hdr):
            with tempfile.TemporaryDirectory(dir=d) as td:
                src, tmp = os.path.join(td, "shim.c"), os.path.join(td, "shim.so")
                open(src, "w").write(_SHIM_SRC)
                subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), src, "-o", tmp, "-lm"])
                os.replace(tmp, so)
        L = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        L.e2e_sincosf.argtypes = [fp, fp, fp, C.c_int]
        L.e2e_sincosf.restype = None
        _SHIM = L
    return _SHIM


def sincosf(x):
    x = np.ascontiguousarray(x, f32).ravel()
    s, c = np.zeros_like(x), np.zeros_like(x)
    fp = C.POINTER(C.c_float)
    _shim().e2e_sincosf(x.ctypes.data_as(fp), s.ctypes.data_as(fp), c.ctypes.data_as(fp), len(x))
    return s, c


class Track:
    """the parts of the track table the restatements read (config.make_config's float32 copies)"""

    def __init__(self, built):
        cfg = built.cfg
        self.L = cfg.num_sections
        sec = [built.sections[i] for i in range(self.L)]
        self.trig_x = np.array([s.trig_x for s in sec], f32)
        self.trig_z = np.array([s.trig_z for s in sec], f32)
        self.marker_y = np.array([s.marker_y for s in sec], f32)
        self.lane_x = np.array([list(s.lane_x) for s in sec], f32)
        self.lane_z = np.array([list(s.lane_z) for s in sec], f32)
        self.straight = np.array([s.track_inside_radius == 0.0 for s in sec])
        self.H, self.laps, self.max_lc = cfg.section_horizon, cfg.laps, cfg.max_lane_changes
        self.kart_y = f32(cfg.kart_y)
        st = cfg.stats
        self.top, self.rev, self.max_steer, self.min_steer = f32(st.TopSpeed), f32(st.ReverseSpeed), f32(st.MaxSteer), f32(st.MinSteer)
        rw = cfg.rw
        self.towards, self.accel_rw, self.speed_rw = f32(rw.TowardsCheckpointReward), f32(rw.AccelerationReward), f32(rw.SpeedReward)

    def marker(self, idx, lane):
        """DPT.getBoxColliderForLane: lane 0 -> the Trigger"""
        if lane == 0:
            return self.trig_x[idx], self.trig_z[idx]
        return self.lane_x[idx, lane - 1], self.lane_z[idx, lane - 1]


def _mag3(x, y, z):
    return f32(np.sqrt(f32(f32(f32(x * x) + f32(y * y)) + f32(z * z))))


def local_speed(tr, a, fx, fz):
    """ArcadeKart.LocalSpeed AK:325-342"""
    from hierarchicalkarting_amd import _lib
    if not (int(a["flags"]) & _lib.HK_F_CAN_MOVE):
        return f32(0.0)
    vx, vz = f32(a["vx"]), f32(a["vz"])
    dot = f32(f32(fx * vx) + f32(fz * vz))
    if abs(dot) > f32(0.1):
        speed = _mag3(vx, f32(0.0), vz)
        return f32(-(speed / tr.rev)) if dot < 0 else f32(speed / tr.top)
    return f32(0.0)


def inv_transform_point(apx, apz, fx, fz, wx, wy, wz, ky):
    rx, rz = f32(wx - apx), f32(wz - apz)
    return [f32(f32(rx * fz) + f32(rz * f32(-fx))), f32(wy - ky), f32(f32(rx * fx) + f32(rz * fz))]


def observe_e2e(tr, a, n_others):
    """own block (8) and section horizon (5 x H) of one E2E kart's observation; returns (own, horizon) as float32 arrays"""
    from hierarchicalkarting_amd import _lib
    fx, fz = sincosf([a["yaw"]])
    fx, fz = fx[0], fz[0]
    fl = int(a["flags"])
    sec = int(a["section_index"])
    goal = f32(tr.laps * tr.L + 1)
    own = np.array([local_speed(tr, a, fx, fz), 1.0 if fl & _lib.HK_F_ACCEL else 0.0, f32(int(a["lane"])),
                    f32(f32(f32(int(a["lane_changes"])) * f32(1.0)) / f32(tr.max_lc)), 1.0 if fl & _lib.HK_F_ACTIVE else 0.0,
                    1.0 if tr.straight[sec % tr.L] else 0.0,
                    f32(f32(tr.max_steer - f32(a["final_steer"])) / f32(tr.max_steer - tr.min_steer)),
                    f32(f32(f32(sec) * f32(1.0)) / goal)], f32)
    hz = []
    for q in range(tr.H):
        nxt = (sec + 1 + q) % tr.L
        hz += inv_transform_point(f32(a["px"]), f32(a["pz"]), fx, fz, tr.trig_x[nxt], tr.marker_y[nxt], tr.trig_z[nxt], tr.kart_y)
        hz += [f32(1.0), f32(1.0) if tr.straight[nxt] else f32(0.0)]
    return own, np.array(hz, f32)


def obs_layout(A, H):
    """index ranges of the blocks of one observation row: (own, others, horizon, rays)"""
    o = 8 + 12 * (A - 1)
    return slice(0, 8), slice(8, o), slice(o, o + 5 * H), slice(o + 5 * H, o + 5 * H + 9)


def academy_e2e(tr, a, branch):
    """the rewards E2E OnActionReceived adds on the state `a` the previous tick left, decoded from discrete action `branch`, in the
    order they are added; -> their float32 running sum starting from 0 (the agent's m_Reward right after hk_get_rewards)"""
    from hierarchicalkarting_amd import _lib
    fl = int(a["flags"])
    if not (fl & _lib.HK_F_ENABLED) or not (fl & _lib.HK_F_ACTIVE):
        return f32(0.0)
    accel, brake = branch > 1, branch < 1
    fx, fz = sincosf([a["yaw"]])
    ls = local_speed(tr, a, fx[0], fz[0])
    nxt = (int(a["section_index"]) + 1) % tr.L
    acc = f32(0.0)
    for target_lane in (int(a["plan_lane"][nxt]), 0):     # base KartAgent.OnActionReceived (plan lane box), then E2E:400-414 (the Trigger)
        cx, cz = tr.marker(nxt, target_lane)
        dx, dy, dz = f32(cx - f32(a["px"])), f32(tr.marker_y[nxt] - tr.kart_y), f32(cz - f32(a["pz"]))
        dm = _mag3(dx, dy, dz)
        if dm > f32(1e-5):
            dx, dy, dz = f32(dx / dm), f32(dy / dm), f32(dz / dm)
        else:
            dx = dy = dz = f32(0.0)
        vx, vy, vz = f32(a["vx"]), f32(0.0), f32(a["vz"])
        vm = _mag3(vx, vy, vz)
        if vm > f32(1e-5):
            vx, vy, vz = f32(vx / vm), f32(vy / vm), f32(vz / vm)
        else:
            vx = vy = vz = f32(0.0)
        rew = f32(f32(f32(vx * dx) + f32(vy * dy)) + f32(vz * dz))
        acc = f32(acc + f32(rew * tr.towards))
        acc = f32(acc + f32(f32(1.0 if (accel and not brake) else 0.0) * tr.accel_rw))
        acc = f32(acc + f32(f32(f32(ls - f32(0.0)) / f32(1.0 - f32(0.0))) * tr.speed_rw))
    return acc
