"""The sensor fit of the ingestion (``ops.fit_events``) restated sequentially: ``map_pixel`` is the rule's steps 1 to 4
for one pixel in plain Python integers, ``Fit`` is one loop over the events, one at a time, with the state block in the op's layout;
``feed`` takes chunks of a stream and carries the state -- the accumulators of ``fire`` included -- as the op does."""
import numpy as np

from filter_ref import OrderError, records, unpack  # noqa: F401  (the record helpers are those of the activity filter's restatement)

STATE_HEAD = 8
COUNTERS = ('seen', 'kept', 'outside', 'cropped', 'skipped', 'merged')
REDUCES = ('pick', 'sum', 'fire')
ORIENTS = (0, 90, 180, 270)


def oriented_hw(src_hw, orient):
    hs, ws = src_hw
    return (ws, hs) if orient in (90, 270) else (hs, ws)


def orient_pixel(x, y, src_hw, orient=0, mirror=False):
    """Steps 1 and 2: a pixel of the sensor -> (x', y') in the image of size ``oriented_hw``."""
    hs, ws = src_hw
    if mirror:
        x = ws - 1 - x
    if orient == 90:
        return hs - 1 - y, x
    if orient == 180:
        return ws - 1 - x, hs - 1 - y
    if orient == 270:
        return y, ws - 1 - x
    assert orient == 0
    return x, y


def map_pixel(x, y, src_hw, dst_hw, orient=0, mirror=False, scale=1, offset=(0, 0)):
    """A pixel inside the sensor -> ('cropped', None, None) or (None, xd, yd) with the remainder (x' % k, y' % k) as a fourth entry."""
    k = scale
    xo, yo = orient_pixel(x, y, src_hw, orient, mirror)
    ho, wo = oriented_hw(src_hw, orient)
    if xo >= (wo // k) * k or yo >= (ho // k) * k:
        return 'cropped', None, None, None
    xd, yd = xo // k + offset[0], yo // k + offset[1]
    if not (0 <= xd < dst_hw[1] and 0 <= yd < dst_hw[0]):
        return 'cropped', None, None, None
    return None, xd, yd, (xo % k, yo % k)


class Fit:
    def __init__(self, src_hw, dst_hw, orient=0, mirror=False, scale=1, offset=(0, 0), reduce='pick', threshold=None):
        assert reduce in REDUCES and orient in ORIENTS and scale >= 1
        self.src, self.dst = tuple(src_hw), tuple(dst_hw)
        self.geo = dict(orient=orient, mirror=mirror, scale=scale, offset=tuple(offset))
        self.k, self.reduce = scale, reduce
        self.theta = (scale * scale if threshold is None else threshold) if reduce == 'fire' else None
        self.acc = [0] * (self.dst[0] * self.dst[1])
        self.t_last = -1
        for c in COUNTERS:
            setattr(self, c, 0)
        self.max_abs = 0                                         # the largest |a| an accumulator held after an event

    def feed(self, rec) -> np.ndarray:
        """A chunk of records [n, 2] -> the kept ones with the mapped coordinates, in order.  A decreasing time raises before anything is
        changed."""
        rec = np.asarray(rec, dtype='<u4').reshape(-1, 2)
        ts, xs, ys, ps = (a.tolist() for a in unpack(rec))
        words = rec[:, 1].tolist()
        before = self.t_last
        for i, t in enumerate(ts):
            if t < before:
                raise OrderError(i, before, t)
            before = t
        out = []
        for t, x, y, p, word in zip(ts, xs, ys, ps, words):
            self.seen += 1
            self.t_last = t
            if x >= self.src[1] or y >= self.src[0]:
                self.outside += 1
                continue
            why, xd, yd, rem = map_pixel(x, y, self.src, self.dst, **self.geo)
            if why is not None:
                self.cropped += 1
                continue
            if self.reduce == 'pick' and rem != (self.k // 2, self.k // 2):
                self.skipped += 1
                continue
            if self.reduce == 'fire':
                q = yd * self.dst[1] + xd
                a = self.acc[q] + (1 if p else -1)
                fired = a == self.theta or a == -self.theta
                self.acc[q] = 0 if fired else a
                self.max_abs = max(self.max_abs, abs(self.acc[q]))
                if not fired:
                    self.merged += 1
                    continue
            self.kept += 1
            out.append((t, (word & 0xf0000000) | (yd << 14) | xd))
        return np.array(out, dtype='<u4').reshape(-1, 2)

    def counters(self) -> dict:
        return {c: getattr(self, c) for c in COUNTERS}

    def state(self) -> list:
        """The op's state block (include/leod_hip.h): the six counters, the last time seen, a zero, the accumulators."""
        return [self.seen, self.kept, self.outside, self.cropped, self.skipped, self.merged, self.t_last, 0] + list(self.acc)
