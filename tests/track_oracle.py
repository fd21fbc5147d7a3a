"""Feature tracks restated with dicts and loops (include/viso_hip.h: vh_track): sequential and obviously correct rather
than fast.  What tests/test_tracks.py compares the GPU linking against, byte for byte.

Link rule: record j of a list continues record q of its predecessor list iff i1p(j) >= 0 and i1c(q) == i1p(j); of several
q the lowest; a predecessor record is continued by the lowest such j only.  Indices outside [0, n_index) never link.
Every other record starts a new track."""
import numpy as np

TRACK = np.dtype([("birth_frame", "<i8"), ("birth_pos", "<i4"), ("age", "<i4"), ("prev", "<i4"), ("reserved", "<i4")])


def link_one(pm, pred, n_index, serial):
    """Tracks of the list `pm` (records with i1p, i1c) whose frame B has the serial `serial`;
    pred = (i1c array, TRACK array) of the predecessor list, or None."""
    out = np.zeros(len(pm), TRACK)
    first_q = {}
    if pred is not None:
        for q, c in enumerate(pred[0]):
            c = int(c)
            if 0 <= c < n_index and c not in first_q:
                first_q[c] = q
    claimed = set()
    for j in range(len(pm)):
        p = int(pm["i1p"][j])
        prev = -1
        if 0 <= p < n_index and p in first_q and first_q[p] not in claimed:
            prev = first_q[p]
            claimed.add(prev)
        if prev < 0:
            out[j] = (serial, j, 1, -1, 0)
        else:
            t = pred[1][prev]
            out[j] = (t["birth_frame"], t["birth_pos"], t["age"] + 1, prev, 0)
    return out


class Carry:
    def __init__(self, pred=None, next_serial=0):
        self.pred, self.next_serial = pred, next_serial


def link(lists, n_index, carry=None):
    """vh_link_tracks: list l continues list l - 1, list 0 the carry's list -> ([tracks], carry)."""
    pred = carry.pred if carry is not None else None
    serial = carry.next_serial if carry is not None else 0
    out = []
    for pm in lists:
        trk = link_one(pm, pred, n_index, serial)
        out.append(trk)
        pred = (np.array(pm["i1c"], np.int64), trk)
        serial += 1
    return out, Carry(pred, serial)


class Camera:
    """The predecessor rule of a stateful handle for one camera (a lone matcher, a stream of a group, or the frames of a
    sequence handle taken one by one): push() per pushed frame, match() per match call on the current pair."""

    def __init__(self, n_index=1 << 24):
        self.n_index = n_index
        self.restart()

    def restart(self):
        """A change of dims: the ring restarts, serials count from 0 again."""
        self.serial, self.pred, self.cur = -1, None, None

    def push(self, replace=False):
        if self.serial < 0:
            self.serial = 0
        elif replace:
            self.cur = None            # the pair has a new frame B (or, next step, a new frame A): its list is void
        else:
            self.serial += 1
            self.pred, self.cur = self.cur, None

    def match(self, pm):
        trk = link_one(pm, self.pred, self.n_index, self.serial)
        self.cur = (np.array(pm["i1c"], np.int64), trk)
        return trk
