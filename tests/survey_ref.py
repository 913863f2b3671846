"""The filter survey of the ingestion (``ops.survey_events``) restated sequentially: ``Survey`` is one loop over the
records that follows the definitions sentence by sentence -- a timestamp surface for the neighbour interval, and per pixel the previous
candidate, the last rising edge, the previous candidate's bin and the uncapped (lock = 255) run of in-band periods -- with the state
block in the op's layout; ``feed`` takes chunks of a stream and carries the state, as the op does.  ``bin_of`` is a plain count, not a
search.  The restatement is checked against the filters' own restatements through the five identities (tests/test_survey_cpu.py)."""
import numpy as np

from filter_ref import OrderError, records, unpack  # noqa: F401  (the record helpers are those of the activity filter's restatement)

NEVER = -1
INF = 255                                                        # "no same-polarity predecessor": above every bin (K <= 64)
STATE_HEAD = 8
PIXEL_LONGS = 4
RUN_BINS = 256
HEAD = ('seen', 'candidates', 'outside', 'masked', 't_first', 't_last')


def bin_of(edges, d):
    """The number of edges < d."""
    return sum(1 for e in edges if e < d)


class Survey:
    def __init__(self, height, width, edges_us, flicker=None, mask=None):
        self.h, self.w = int(height), int(width)
        self.edges = [int(e) for e in edges_us]
        assert 1 <= len(self.edges) <= 64 and all(0 <= e < 2 ** 31 for e in self.edges)
        assert all(a < b for a, b in zip(self.edges[:-1], self.edges[1:]))
        self.band = None if flicker is None else (int(flicker[0]), int(flicker[1]))
        self.mask = None if mask is None else (np.asarray(mask).reshape(self.h, self.w) != 0)
        K, n = len(self.edges), self.h * self.w
        self.K = K
        self.seen = self.candidates = self.outside = self.masked = 0
        self.t_first = self.t_last = NEVER
        self.nb, self.same, self.sec_on, self.sec_off = [0] * (K + 2), [0] * (K + 1), [0] * (K + 1), [0] * (K + 1)
        self.period, self.run = [0] * (K + 1), [0] * RUN_BINS
        self.t_prev, self.t_edge, self.p_prev, self.c_prev, self.n_per = [NEVER] * n, [NEVER] * n, [0] * n, [INF] * n, [0] * n
        # the neighbours of every pixel that lie inside the sensor; the pixel itself is none of them
        self.nbs = [[(y + dy) * self.w + x + dx for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                     if (dx or dy) and 0 <= x + dx < self.w and 0 <= y + dy < self.h] for y in range(self.h) for x in range(self.w)]

    def feed(self, rec) -> None:
        """A chunk of records [n, 2].  A decreasing time raises before anything is changed."""
        rec = np.asarray(rec, dtype='<u4').reshape(-1, 2)
        ts, xs, ys, ps = (a.tolist() for a in unpack(rec))
        before = self.t_last
        for i, ti in enumerate(ts):
            if ti < before:
                raise OrderError(i, before, ti)
            before = ti
        K, edges = self.K, self.edges
        for i in range(len(ts)):
            t, x, y, p = ts[i], xs[i], ys[i], ps[i]
            self.seen += 1
            if self.t_first == NEVER:
                self.t_first = t
            if x >= self.w or y >= self.h:
                self.outside += 1
                continue
            if self.mask is not None and self.mask[y, x]:
                self.masked += 1
                continue
            self.candidates += 1
            q = y * self.w + x
            # nb: the surface is t_prev of every pixel -- every candidate writes it, below
            latest = max((self.t_prev[r] for r in self.nbs[q]), default=NEVER)
            self.nb[K + 1 if latest == NEVER else bin_of(edges, t - latest)] += 1
            # same, sec_on, sec_off
            first = self.t_prev[q] == NEVER
            c = bin_of(edges, t - self.t_prev[q]) if (not first and p == self.p_prev[q]) else INF
            if c != INF:
                self.same[c] += 1
            c_before = self.c_prev[q]
            if c < c_before and c < K:
                self.sec_on[c] += 1
                if c_before <= K:
                    self.sec_off[c_before] += 1
            # period, run: steps (c) and (d) of the per-pixel rule with lock = 255
            if self.band is not None and self.t_edge[q] != NEVER and t - self.t_edge[q] > self.band[1]:
                self.n_per[q] = 0
            if p == 1 and (first or self.p_prev[q] == 0):
                if self.t_edge[q] != NEVER:
                    d = t - self.t_edge[q]
                    self.period[bin_of(edges, d)] += 1
                    if self.band is not None:
                        self.n_per[q] = min(self.n_per[q] + 1, 255) if self.band[0] <= d <= self.band[1] else 0
                self.t_edge[q] = t
            if self.band is not None:
                self.run[self.n_per[q]] += 1
            self.t_prev[q], self.p_prev[q], self.c_prev[q] = t, p, c
        if len(ts):
            self.t_last = ts[-1]

    def counters(self) -> dict:
        out = {k: getattr(self, k) for k in HEAD}
        for k in ('nb', 'same', 'sec_on', 'sec_off', 'period', 'run'):
            out[k] = np.asarray(getattr(self, k), dtype=np.int64)
        return out

    def state(self) -> list:
        """The op's state block (include/leod_hip.h): the head, the histograms, then t_prev, t_edge, p_prev + 2 * c_prev, n_per of every
        pixel."""
        out = [self.seen, self.candidates, self.outside, self.masked, self.t_first, self.t_last, 0, 0]
        out += self.nb + self.same + self.sec_on + self.sec_off + self.period + self.run
        for q in range(self.h * self.w):
            out += [self.t_prev[q], self.t_edge[q], self.p_prev[q] + 2 * self.c_prev[q], self.n_per[q]]
        return out
