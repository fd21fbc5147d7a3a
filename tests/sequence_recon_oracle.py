"""Reconstruction from tracked lists restated with loops (include/viso_hip.h: vh_sequence_reconstruct, vh_reconstruct_lists;
DESIGN.md section 4.8) -- test infrastructure, sequential and obviously correct rather than fast.

Linking is track_oracle.link_one (the link rule), a lost track's point is reconstruction_oracle.solve_track on
reconstruction_oracle.Tables.  A Drive is the state of one handle: chunk() is one vh_sequence_reconstruct, reset() is a
break (a new Reconstruction constructed at the frame before the next list)."""
import numpy as np

import reconstruction_oracle as ro
import track_oracle as to

HISTORY = 6
RECON_TRACK = np.dtype([("birth_frame", "<i8"), ("birth_pos", "<i4"), ("frames", "<i4"), ("lost_frame", "<i8"), ("status", "<i4"),
                        ("point", "<f4", (3,)), ("distance", "<f8"), ("angle", "<f8")])


class Drive:
    def __init__(self, svd, cal, history, n_index=1 << 24, point_type=1, min_track_length=2, max_dist=30.0, min_angle=2.0):
        self.svd, self.cal, self.H, self.n_index = svd, cal, int(history), n_index
        self.thresholds = (point_type, min_track_length, max_dist, min_angle)
        self.reset()

    def reset(self):
        """A break: pending tracks and the history are dropped; the next list starts a new Reconstruction."""
        self.tab, self.origin, self.lists, self.last = None, None, {}, None

    def _lost(self, f, q):
        """Record q of the list of frame f - 1 is continued by nothing in the list of frame f."""
        pm, trk = self.lists[f - 1]
        age, bf, bp = int(trk["age"][q]), int(trk["birth_frame"][q]), int(trk["birth_pos"][q])
        rec = np.zeros((), RECON_TRACK)
        rec["birth_frame"], rec["birth_pos"], rec["frames"], rec["lost_frame"] = bf, bp, age + 1, f
        if age > self.H:
            rec["status"] = HISTORY
            return rec
        px, g, pos = [], f - 1, q
        for _ in range(age):
            m, t = self.lists[g]
            px.append((m["u1c"][pos], m["v1c"][pos]))
            if t["prev"][pos] < 0:
                px.append((m["u1p"][pos], m["v1p"][pos]))
            pos, g = int(t["prev"][pos]), g - 1
        assert pos == -1 and g == bf - 1 and len(px) == age + 1
        px.reverse()
        p, status, dist, angle = ro.solve_track(self.tab, self.svd, bf - 1 - self.origin, px, *self.thresholds)
        rec["status"], rec["point"], rec["distance"], rec["angle"] = status, p, dist, angle
        return rec

    def chunk(self, first_frame, lists, Trs):
        """The lists of frames first_frame, first_frame + 1, .. and the Tr of each -> sorted RECON_TRACK records."""
        out = []
        for k, (pm, Tr) in enumerate(zip(lists, Trs)):
            f = first_frame + k
            if self.tab is None:
                self.tab, self.origin = ro.Tables(*self.cal), f - 1
            assert self.last is None or self.last == f - 1, "chunks continue each other, or reset() comes first"
            self.tab.push(Tr)
            pred = self.lists.get(f - 1)
            trk = to.link_one(pm, (np.array(pred[0]["i1c"], np.int64), pred[1]) if pred is not None else None, self.n_index, f)
            self.lists[f] = (pm, trk)
            self.lists.pop(f - self.H - 2, None)
            self.last = f
            if pred is not None:
                kept = set(int(x) for x in trk["prev"] if x >= 0)
                out += [self._lost(f, q) for q in range(len(pred[0])) if q not in kept]
        out.sort(key=lambda r: (int(r["lost_frame"]), int(r["birth_frame"]), int(r["birth_pos"])))
        return np.array(out, RECON_TRACK) if out else np.zeros(0, RECON_TRACK)


def run(svd, cal, lists, Trs, history, T, **kw):
    """A drive of len(lists) + 1 frames pushed in chunks of T frames: lists[k] is the list of frame k + 1.
    -> [records of the chunk] per chunk (the first chunk's row 0 holds no pair)."""
    d, out, N = Drive(svd, cal, history, **kw), [], len(lists) + 1
    for F in range(0, N, T):
        lo, hi = max(F, 1), min(F + T, N)
        out.append(d.chunk(lo, lists[lo - 1:hi - 1], Trs[lo - 1:hi - 1]))
    return out


def whole(svd, cal, lists, Trs, n_index=1 << 24, **kw):
    """vh_reconstruct_lists: one fresh drive, nothing older than the history."""
    return Drive(svd, cal, len(lists), n_index, **kw).chunk(1, lists, Trs)
