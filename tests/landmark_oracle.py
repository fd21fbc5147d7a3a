"""Landmarks (include/viso_hip.h): a numpy restatement of the per-record rule, one Python loop per
record, plain double arithmetic in the order the header states it -- every product and sum rounded on its own, sums added
left to right.  The chain of sums of one track is sequential over the steps and independent of every other record, so the
library is held to these bytes without a tolerance."""
import numpy as np

TRACK = np.dtype([("birth_frame", "<i8"), ("birth_pos", "<i4"), ("age", "<i4"), ("prev", "<i4"), ("reserved", "<i4")])
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("sigma_z", "<f4"), ("err", "<f4"), ("src_pos", "<i4"), ("i1p", "<i4"),
                  ("i1c", "<i4")])
STATE = np.dtype([("sw", "<f8"), ("swx", "<f8"), ("swy", "<f8"), ("swz", "<f8"), ("n_obs", "<i4"), ("n_missed", "<i4"),
                  ("reserved", "<i4", (2,))])
LANDMARK = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("sigma", "<f4"), ("n_obs", "<i4"), ("age", "<i4"),
                     ("birth_frame", "<i8"), ("birth_pos", "<i4"), ("src_pos", "<i4"), ("i1c", "<i4"), ("point_pos", "<i4")])
assert STATE.itemsize == 48 and LANDMARK.itemsize == 48 and POINT.itemsize == 32 and TRACK.itemsize == 24


def params(min_obs=2, max_missed=3, max_dist=0.0, gate_sigma=0.0):
    return dict(min_obs=int(min_obs), max_missed=int(max_missed), max_dist=float(max_dist), gate_sigma=float(gate_sigma))


def update(trk, pts, prev, lp, events=None):
    """One step of one list: trk [n] TRACK, pts [m] POINT (src_pos strictly increasing in [0, n)), prev None or [n_prev]
    STATE -> (landmarks [k] LANDMARK in list order, state_out [n] STATE).  events (a dict, optional) counts the gate
    restarts ("restart"), the max_missed drops ("drop") and the non-finite resets ("nonfinite")."""
    f8 = np.float64
    n = len(trk)
    state = np.zeros(n, STATE)
    out = []
    obs = {int(p["src_pos"]): k for k, p in enumerate(pts)}
    assert len(obs) == len(pts)
    ev = events if events is not None else {}
    zero = (f8(0.0), f8(0.0), f8(0.0), f8(0.0), 0, 0)
    with np.errstate(all="ignore"):
        for j in range(n):
            q = int(trk["prev"][j])
            if prev is not None and 0 <= q < len(prev):                        # 1. carry
                s = prev[q]
                sw, swx, swy, swz, n_obs, n_missed = f8(s["sw"]), f8(s["swx"]), f8(s["swy"]), f8(s["swz"]), int(s["n_obs"]), int(s["n_missed"])
            else:
                sw, swx, swy, swz, n_obs, n_missed = zero
            k = obs.get(j)
            emit = False
            if k is None:                                                      # 2. no observation
                if n_obs > 0:
                    n_missed += 1
                    if lp["max_missed"] >= 0 and n_missed > lp["max_missed"]:
                        sw, swx, swy, swz, n_obs, n_missed = zero
                        ev["drop"] = ev.get("drop", 0) + 1
            else:                                                              # 3. the observation
                x, y, z, sg = f8(pts["x"][k]), f8(pts["y"][k]), f8(pts["z"][k]), f8(pts["sigma_z"][k])
                w = f8(1.0) / (sg * sg) if sg > 0 else f8(1.0)
                if n_obs > 0:
                    T = f8(lp["max_dist"]) + f8(lp["gate_sigma"]) * sg
                    if T > 0:
                        dx = x - swx / sw; dy = y - swy / sw; dz = z - swz / sw
                        if dx * dx + dy * dy + dz * dz > T * T:
                            sw, swx, swy, swz, n_obs, n_missed = zero
                            ev["restart"] = ev.get("restart", 0) + 1
                sw = sw + w; swx = swx + w * x; swy = swy + w * y; swz = swz + w * z
                n_obs += 1; n_missed = 0
                if not (np.isfinite(sw) and np.isfinite(swx) and np.isfinite(swy) and np.isfinite(swz)):
                    sw, swx, swy, swz, n_obs, n_missed = zero
                    ev["nonfinite"] = ev.get("nonfinite", 0) + 1
                else:
                    emit = n_obs >= lp["min_obs"]                              # 5.
            state[j] = (sw, swx, swy, swz, n_obs, n_missed, (0, 0))            # 4.
            if emit:
                out.append((np.float32(swx / sw), np.float32(swy / sw), np.float32(swz / sw), np.float32(np.sqrt(f8(1.0) / sw)),
                            n_obs, int(trk["age"][j]), int(trk["birth_frame"][j]), int(trk["birth_pos"][j]), j, int(pts["i1c"][k]), k))
    return np.array(out, LANDMARK).reshape(-1), state


def update_lists(tracks, points, prev, lp, events=None):
    """The step for several independent lists -> ([landmarks per list], [state per list])."""
    res = [update(t, p, None if prev is None else prev[s], lp, events) for s, (t, p) in enumerate(zip(tracks, points))]
    return [r[0] for r in res], [r[1] for r in res]
