"""The per-pixel event filters of the ingestion (``ops.pixel_filter_events``) restated sequentially: ``PixelFilter``
is one loop that is the rule step by step, with the state block in the op's layout; ``feed`` takes chunks of a stream and carries the
state, as the op does.  ``by_the_sentence`` is an independent transcription that keeps no state at all: the burst position of an event
comes from scanning backwards over the same pixel's earlier candidates, the flicker count from recomputing over the pixel's full list
of rising edges.  The restatement is checked against it (tests/test_pixfilter_cpu.py)."""
import numpy as np

from filter_ref import OrderError, records, unpack  # noqa: F401  (the record helpers are those of the activity filter's restatement)

NEVER = -1
STATE_HEAD = 8
PIXEL_LONGS = 4
COUNTERS = ('seen', 'kept', 'outside', 'masked', 'flicker', 'burst')
KEEP = ('first', 'second', 'from_second')


def position_passes(burst_keep, k):
    return {'first': k == 1, 'second': k == 2, 'from_second': k >= 2}[burst_keep]


class PixelFilter:
    """Per pixel: t_prev, p_prev, k_prev, t_edge, n_per; the time of the last event seen; the six counters; and the loop."""

    def __init__(self, height, width, burst_us=None, burst_keep='first', flicker=None, mask=None):
        assert burst_keep in KEEP
        self.h, self.w, self.tau, self.keep, self.flicker = int(height), int(width), burst_us, burst_keep, flicker
        self.mask = None if mask is None else (np.asarray(mask).reshape(self.h, self.w) != 0)
        n = self.h * self.w
        self.t_prev, self.p_prev, self.k_prev, self.t_edge, self.n_per = [NEVER] * n, [0] * n, [0] * n, [NEVER] * n, [0] * n
        self.t_last = NEVER
        self.seen = self.kept = self.outside = self.masked = self.n_flicker = self.n_burst = 0

    def feed(self, rec) -> np.ndarray:
        """A chunk of records [n, 2] -> the kept ones, unchanged and in order.  A decreasing time raises before anything is changed."""
        rec = np.asarray(rec, dtype='<u4').reshape(-1, 2)
        ts, xs, ys, ps = (a.tolist() for a in unpack(rec))
        before = self.t_last
        for i, ti in enumerate(ts):
            if ti < before:
                raise OrderError(i, before, ti)
            before = ti
        keep = []
        tau, fl = self.tau, self.flicker
        for i in range(len(ts)):
            t, x, y, p = ts[i], xs[i], ys[i], ps[i]
            self.seen += 1
            if x >= self.w or y >= self.h:                       # 1
                self.outside += 1
                continue
            if self.mask is not None and self.mask[y, x]:        # 2
                self.masked += 1
                continue
            q = y * self.w + x                                   # 3: a candidate
            first = self.t_prev[q] == NEVER                      # (a)
            connected = tau is not None and not first and p == self.p_prev[q] and t - self.t_prev[q] <= tau      # (b)
            k = min(self.k_prev[q] + 1, 3) if connected else 1
            if fl is not None:
                p_min, p_max, lock = fl
                if self.t_edge[q] != NEVER and t - self.t_edge[q] > p_max:       # (c)
                    self.n_per[q] = 0
                if p == 1 and (first or self.p_prev[q] == 0):                    # (d)
                    if self.t_edge[q] != NEVER:
                        d = t - self.t_edge[q]
                        self.n_per[q] = min(self.n_per[q] + 1, lock) if p_min <= d <= p_max else 0
                    self.t_edge[q] = t
            self.t_prev[q], self.p_prev[q], self.k_prev[q] = t, p, k             # (e)
            if fl is not None and self.n_per[q] >= fl[2]:                        # (f)
                self.n_flicker += 1
            elif tau is not None and not position_passes(self.keep, k):
                self.n_burst += 1
            else:
                self.kept += 1
                keep.append(i)
        if len(ts):
            self.t_last = ts[-1]
        return rec[keep]

    def counters(self) -> dict:
        return dict(seen=self.seen, kept=self.kept, outside=self.outside, masked=self.masked, flicker=self.n_flicker, burst=self.n_burst)

    def state(self) -> list:
        """The op's state block (include/leod_hip.h): the head, then t_prev, t_edge, p_prev + 2 * k_prev, n_per of every pixel."""
        out = [self.seen, self.kept, self.outside, self.masked, self.n_flicker, self.n_burst, self.t_last, 0]
        for q in range(self.h * self.w):
            out += [self.t_prev[q], self.t_edge[q], self.p_prev[q] + 2 * self.k_prev[q], self.n_per[q]]
        return out


def by_the_sentence(rec, height, width, burst_us=None, burst_keep='first', flicker=None, mask=None):
    """-> (indices of the kept events, dict of the counters), with no state carried from event to event.
    Burst position of candidate c: walk back over the pixel's candidates while each one is connected to the one before it (same
    polarity, at most tau apart); the position is the length of that chain, counted up to 3.
    Flicker count at candidate c: take the pixel's rising edges up to and including c (an ON candidate whose predecessor on the pixel
    is OFF or absent); the count is the number of trailing consecutive in-band periods between them, capped at lock -- unless some
    candidate up to c, lying after the last edge, came later than p_max behind it: that one reset the count to 0, and no edge has
    followed to raise it (an edge later than p_max is out of band and itself counts as a reset)."""
    t, x, y, p = (a.tolist() for a in unpack(rec))
    n = len(t)
    m = None if mask is None else (np.asarray(mask).reshape(height, width) != 0)
    cand_of = {}                                                 # pixel -> the indices of its candidates, in stream order
    counts = dict(seen=n, kept=0, outside=0, masked=0, flicker=0, burst=0)
    kept = []
    for i in range(n):
        if x[i] >= width or y[i] >= height:
            counts['outside'] += 1
            continue
        if m is not None and m[y[i], x[i]]:
            counts['masked'] += 1
            continue
        c = cand_of.setdefault(y[i] * width + x[i], [])
        c.append(i)
        # burst position
        k = 1
        if burst_us is not None:
            j = len(c) - 1
            while j > 0 and p[c[j]] == p[c[j - 1]] and t[c[j]] - t[c[j - 1]] <= burst_us:
                k += 1
                j -= 1
            k = min(k, 3)
        # flicker count
        locked = False
        if flicker is not None:
            p_min, p_max, lock = flicker
            edges = [c[j] for j in range(len(c)) if p[c[j]] == 1 and (j == 0 or p[c[j - 1]] == 0)]
            n_per = 0
            if edges:
                run = 0
                for a, b in zip(edges[:-1], edges[1:]):
                    run = run + 1 if p_min <= t[b] - t[a] <= p_max else 0
                n_per = min(run, lock)
                # Saturation loses nothing: min(n + 1, lock) step by step equals min(run, lock).  A timeout between two edges is covered
                # by the next edge, which is then out of band (d > p_max); only one after the last edge is left to look for.
                if any(t[j] - t[edges[-1]] > p_max for j in c if j > edges[-1]):
                    n_per = 0
            locked = n_per >= lock
        if locked:
            counts['flicker'] += 1
        elif burst_us is not None and not position_passes(burst_keep, k):
            counts['burst'] += 1
        else:
            counts['kept'] += 1
            kept.append(i)
    return np.asarray(kept, dtype=np.int64), counts


def lamp_stream(rng, n, height, width, lamps, outside=0.03, period=10_000, jitter=300, clear_lamps=False):
    """A random stream of n events: a uniform background over t in [0, 40 n] with ``outside`` of the events beyond the sensor, and on each
    of the ``lamps`` pixels (x, y) a flickering source of the given period: two ON events at the start of every cycle and two OFF events
    half a cycle later, each time jittered.  ``clear_lamps``: the background stays off the lamp pixels, so they lock for certain.
    -> records [n, 2], sorted in time (stable: equal times keep the order of generation)."""
    t_max = 40 * n
    parts = []
    for lx, ly in lamps:
        starts = np.arange(500, t_max - period, period)
        for half, pol in ((0, 1), (period // 2, 0)):
            for rep in range(2):
                tt = starts + half + rep * 40 + rng.randint(-jitter, jitter + 1, len(starts))
                parts.append((tt, np.full(len(tt), lx), np.full(len(tt), ly), np.full(len(tt), pol)))
    n_lamp = sum(len(q[0]) for q in parts)
    n_bg = n - n_lamp
    assert n_bg >= 0, (n, n_lamp)
    bx, by = rng.randint(0, width, n_bg), rng.randint(0, height, n_bg)
    if clear_lamps:
        for lx, ly in lamps:
            hit = (bx == lx) & (by == ly)
            bx[hit] = (lx + 1) % width
    out = rng.rand(n_bg) < outside
    bx[out] += width
    parts.append((rng.randint(0, t_max, n_bg), bx, by, rng.randint(0, 2, n_bg)))
    t, x, y, p = (np.concatenate([q[k] for q in parts]).astype(np.int64) for k in range(4))
    t = np.clip(t, 0, None)
    order = np.argsort(t, kind='stable')
    return records(t[order], x[order], y[order], p[order])
