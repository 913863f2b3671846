"""The event noise filter of the ingestion (``ops.filter_events``) restated sequentially: one loop over the records
and a timestamp surface.  ``Filter.feed`` takes chunks of a stream and carries the state, as the op does; ``by_the_sentence`` is the
O(n^2) transcription of the rule's sentence that the restatement itself is checked against (tests/test_event_filter_cpu.py)."""
import numpy as np

NEVER = -1
STATE_HEAD = 8
COUNTERS = ('seen', 'kept', 'outside', 'masked', 'unsupported')


def records(t, x, y, p=None) -> np.ndarray:
    """(t, x, y, p) -> .dat records [n, 2] u32: t; x in bits 0-13, y in bits 14-27, p in bit 28."""
    t, x, y = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (t, x, y))
    p = np.zeros_like(t) if p is None else np.asarray(p, dtype=np.int64).reshape(-1)
    assert t.min(initial=0) >= 0 and t.max(initial=0) < 2 ** 32 and x.max(initial=0) < 2 ** 14 and y.max(initial=0) < 2 ** 14
    return np.stack([t, x | (y << 14) | (p << 28)], axis=1).astype('<u4')


def unpack(rec):
    rec = np.asarray(rec).reshape(-1, 2).astype(np.int64)
    return rec[:, 0], rec[:, 1] & 16383, (rec[:, 1] >> 14) & 16383, (rec[:, 1] >> 28) & 1


class OrderError(ValueError):
    def __init__(self, position, t_before, t_at):
        super().__init__(f'timestamps decrease at event {position} ({t_before} -> {t_at})')
        self.position, self.t_before, self.t_at = position, t_before, t_at


class Filter:
    """The filter's state -- the last time per pixel (NEVER: none), the time of the last event seen and the five counters -- and the loop."""

    def __init__(self, height, width, tau_us, mask=None):
        self.h, self.w, self.tau = int(height), int(width), tau_us
        self.mask = None if mask is None else (np.asarray(mask).reshape(self.h, self.w) != 0)
        self.last = [NEVER] * (self.h * self.w)
        self.t_last = NEVER
        self.seen = self.kept = self.outside = self.masked = self.unsupported = 0
        # the neighbours of every pixel that lie inside the sensor; the pixel itself is none of them
        self.nb = [[(y + dy) * self.w + x + dx for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                    if (dx or dy) and 0 <= x + dx < self.w and 0 <= y + dy < self.h] for y in range(self.h) for x in range(self.w)]

    def feed(self, rec) -> np.ndarray:
        """A chunk of records [n, 2] -> the kept ones, unchanged and in order.  A decreasing time raises before anything is changed."""
        rec = np.asarray(rec, dtype='<u4').reshape(-1, 2)
        t, x, y, _ = (a.tolist() for a in unpack(rec))
        before = self.t_last
        for i, ti in enumerate(t):
            if ti < before:
                raise OrderError(i, before, ti)
            before = ti
        keep = []
        last, nb, tau, mask, w = self.last, self.nb, self.tau, self.mask, self.w
        for i in range(len(t)):
            self.seen += 1
            if x[i] >= self.w or y[i] >= self.h:                 # rule 1
                self.outside += 1
                continue
            if mask is not None and mask[y[i], x[i]]:            # rule 2
                self.masked += 1
                continue
            pix = y[i] * w + x[i]
            if tau is None:
                ok = True
            else:                                                # rule 3: a neighbour fired at most tau ago (NEVER is no time)
                ok = False
                for q in nb[pix]:
                    if last[q] != NEVER and t[i] - last[q] <= tau:
                        ok = True
                        break
            last[pix] = t[i]                                     # kept or not: the surface takes every event that passed rules 1 and 2
            if ok:
                self.kept += 1
                keep.append(i)
            else:
                self.unsupported += 1
        if len(t):
            self.t_last = t[-1]
        return rec[keep]

    def counters(self) -> dict:
        return {k: getattr(self, k) for k in COUNTERS}

    def state(self) -> list:
        """The op's state block (include/leod_hip.h): counters, last time seen, two zeros, the surface."""
        return [self.seen, self.kept, self.outside, self.masked, self.unsupported, self.t_last, 0, 0] + list(self.last)


def by_the_sentence(rec, height, width, tau_us, mask=None) -> np.ndarray:
    """Indices of the kept events by the rule as it is written: event i is kept iff it is inside the sensor, not masked, and some EARLIER
    event j < i that is inside and not masked lies on one of its 8 neighbours with t_i - t_j <= tau."""
    t, x, y, _ = unpack(rec)
    n = len(t)
    passes = (x < width) & (y < height)
    if mask is not None:
        m = np.asarray(mask).reshape(height, width) != 0
        passes &= ~m[np.minimum(y, height - 1), np.minimum(x, width - 1)]
    kept = []
    for i in range(n):
        if not passes[i]:
            continue
        for j in range(i):
            if passes[j] and max(abs(x[i] - x[j]), abs(y[i] - y[j])) == 1 and t[i] - t[j] <= tau_us:
                kept.append(i)
                break
    return np.asarray(kept, dtype=np.int64)
