"""The video-to-events simulator (``ops.simulate_events``) restated sequentially in plain Python integers: one pixel
at a time, one interval at a time, then the global order (t, pixel, j).  ``Sim.feed`` takes the frames of a call and carries the state as
the op does; ``state`` is the op's state block, word for word."""
import numpy as np

STATE_HEAD = 8
COUNTERS = ('frames', 'kept', 'on', 'off', 'dropped')
MAX_SIDE = 16384
LUT_LIMIT = 1 << 24
MAX_CANDIDATES = 4096
T_LIMIT = 1 << 32


def check(height, width, lut, theta_on, theta_off, refractory_us):
    """``ValueError`` for every limit of the rule but those on the times."""
    for name, v in (('height', height), ('width', width)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_SIDE:
            raise ValueError(f'{name}={v!r}')
    if height * width >= 1 << 30:
        raise ValueError('height * width >= 2^30')
    if np.asarray(lut).dtype.kind not in 'iu':
        raise ValueError('lut: integers expected')
    lut = [int(v) for v in np.asarray(lut).reshape(-1)]
    if len(lut) != 256 or min(lut) < 0 or max(lut) >= LUT_LIMIT:
        raise ValueError('lut')
    least = None
    for name, th in (('theta_on', theta_on), ('theta_off', theta_off)):
        th = np.asarray(th)
        if th.shape != (height, width) or th.dtype.kind not in 'iu':
            raise ValueError(f'{name}: shape {th.shape}, dtype {th.dtype}')
        lo, hi = int(th.min()), int(th.max())
        if lo < 1 or hi >= 1 << 31:
            raise ValueError(f'{name}: values in [{lo}, {hi}]')
        least = lo if least is None else min(least, lo)
    if (max(lut) - min(lut)) // least > MAX_CANDIDATES:
        raise ValueError('more than 4096 candidates per pixel and interval')
    if isinstance(refractory_us, bool) or not isinstance(refractory_us, (int, np.integer)) or not 0 <= refractory_us < T_LIMIT:
        raise ValueError(f'refractory_us={refractory_us!r}')


def check_times(times, t_last):
    if len(times) and np.asarray(times).dtype.kind not in 'iu':
        raise ValueError('times: integers expected')
    times =[int(t) for t in times]
    before = t_last
    for t in times:
        if not 0 <= t < T_LIMIT or t <= before:
            raise ValueError(f'times: {before} is followed by {t}')
        before = t
    return times


def walk_interval(m, t_keep, l0, l1, t0, t1, theta_on, theta_off, refractory_us):
    """One pixel, one interval -> (m, t_keep, [(t, polarity) of the kept candidates], dropped)."""
    kept, dropped, D = [], 0, t1 - t0
    if l1 > l0:
        j = 1
        while m + j * theta_on <= l1:
            t = t0 + max(1, (D * (m + j * theta_on - l0)) // (l1 - l0))
            if t_keep >= 0 and t - t_keep < refractory_us:
                dropped += 1
            else:
                kept.append((t, 1))
                t_keep = t
            j += 1
        m += (j - 1) * theta_on
    elif l1 < l0:
        j = 1
        while m - j * theta_off >= l1:
            t = t0 + max(1, (D * (l0 - (m - j * theta_off))) // (l0 - l1))
            if t_keep >= 0 and t - t_keep < refractory_us:
                dropped += 1
            else:
                kept.append((t, 0))
                t_keep = t
            j += 1
        m -= (j - 1) * theta_off
    return m, t_keep, kept, dropped


class Sim:
    def __init__(self, height, width, lut, theta_on, theta_off, refractory_us=0):
        check(height, width, lut, theta_on, theta_off, refractory_us)
        self.h, self.w, self.refr = int(height), int(width), int(refractory_us)
        self.lut = [int(v) for v in np.asarray(lut).reshape(-1)]
        self.th_on = [int(v) for v in np.asarray(theta_on).reshape(-1)]
        self.th_off = [int(v) for v in np.asarray(theta_off).reshape(-1)]
        P = self.h * self.w
        self.m, self.t_keep, self.last = [0] * P, [-1] * P, [0] * P
        self.frames = self.kept = self.on = self.off = self.dropped = 0
        self.t_last = -1
        self.invariant = True                                    # -theta_off < lut[v] - m < theta_on after every frame, on every pixel
        self.intervals = []                                      # (t0, t1, records of the interval) of every interval fed

    def feed(self, frames, times) -> np.ndarray:
        frames = np.asarray(frames)
        if frames.dtype != np.uint8 or frames.ndim != 3 or frames.shape[1:] != (self.h, self.w):
            raise ValueError(f'frames: {frames.dtype} {frames.shape}')
        times = check_times(times, self.t_last)
        if len(times) != len(frames):
            raise ValueError('one time per frame')
        out = []
        for frame, t1 in zip(frames.reshape(len(frames), self.h * self.w).tolist(), times):
            if self.frames == 0:
                self.m = [self.lut[v] for v in frame]
            else:
                events = []
                for pix, v in enumerate(frame):
                    l0, l1 = self.lut[self.last[pix]], self.lut[v]
                    if l1 == l0:
                        continue
                    m, t_keep, kept, dropped = walk_interval(self.m[pix], self.t_keep[pix], l0, l1, self.t_last, t1, self.th_on[pix],
                                                             self.th_off[pix], self.refr)
                    self.m[pix], self.t_keep[pix] = m, t_keep
                    self.dropped += dropped
                    self.invariant = self.invariant and -self.th_off[pix] < l1 - m < self.th_on[pix]
                    events += [(t, pix, p) for t, p in kept]
                events.sort(key=lambda e: (e[0], e[1]))            # stable: a pixel's candidates of one time stay in the order of j
                self.kept += len(events)
                self.on += sum(e[2] for e in events)
                self.off += sum(1 - e[2] for e in events)
                self.intervals.append((self.t_last, t1, events))
                out += events                                    # intervals never share a time: the stream is the intervals in turn
            self.last, self.t_last = frame, t1
            self.frames += 1
        rec = np.zeros((len(out), 2), dtype='<u4')
        if out:
            t, pix, p = (np.array(c, dtype=np.int64) for c in zip(*out))
            rec[:, 0] = t
            rec[:, 1] = (pix % self.w) | ((pix // self.w) << 14) | (p << 28)
        return rec

    def counters(self):
        return dict(frames=self.frames, kept=self.kept, on=self.on, off=self.off, dropped=self.dropped, t_last=self.t_last)

    def state(self) -> np.ndarray:
        P = self.h * self.w
        tail = np.zeros(((P + 7) // 8 * 8,), dtype=np.uint8)
        tail[:P] = self.last
        per_pixel = np.stack([np.array(self.m, dtype=np.int64), np.array(self.t_keep, dtype=np.int64)], axis=1).reshape(-1)
        head = np.array([self.frames, self.kept, self.on, self.off, self.dropped, self.t_last, 0, 0], dtype=np.int64)
        return np.concatenate([head, per_pixel, tail.view('<i8')])
