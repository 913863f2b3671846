"""A sequential streaming EVT2 / EVT3 encoder, one event at a time as a camera would emit, with an explicit pending group: the tests'
own restatement of the rule of DESIGN.md section 1, written independently of ``raw_events.encode_evt2`` / ``encode_evt3`` (numpy, all events
at once).  Plus the event streams the encoder tests share: hand-written cases and random streams that stress the rule."""
import numpy as np

HIGH_STEP = 1024


class Encoder:
    def __init__(self, fmt: int, vectors: bool = False, high_period: int = 64, first_time_high: int = 0):
        assert fmt in (2, 3) and not (vectors and fmt == 2)
        self.fmt, self.vectors, self.period, self.first = fmt, vectors, max(int(high_period), 1), int(first_time_high)
        self.words = [(0x8 << 28 | self.first) if fmt == 2 else (0x8000 | self.first)]
        self.high, self.low, self.row = self.first, None, None   # what the reader of the words knows after the last word
        self.count = 0                                           # groups (EVT3) or events (EVT2) written
        self.pending = None                                      # EVT3: [time, y, p, [x, ...]] of the group that may still grow
        self.groups = self.vector_groups = 0

    def push(self, t: int, x: int, y: int, p: int) -> None:
        assert 0 <= x < 2048 and 0 <= y < 2048 and p in (0, 1) and t >= 0
        if self.fmt == 2:
            a = t + (self.first << 6)
            if a >> 6 != self.high or self.count % self.period == 0:
                self.high = a >> 6
                self.words.append(0x8 << 28 | self.high)
            self.words.append(p << 28 | (a & 63) << 22 | x << 11 | y)
            self.count += 1
            return
        a = t + (self.first << 12)
        g = self.pending
        if self.vectors and g is not None and g[:3] == [a, y, p] and x > g[3][-1] and x - g[3][0] < 12:
            g[3].append(x)
            return
        self.flush()
        self.pending = [a, y, p, [x]]

    def flush(self) -> None:
        """Writes the pending group out (the end of the recording, or an event that does not continue it)."""
        g, self.pending = self.pending, None
        if g is None:
            return
        a, y, p, xs = g
        high, low = a >> 12, a & 4095
        moved = high > self.high
        if moved:
            while high - self.high > HIGH_STEP:                  # a pause never looks like a wrap of the 12-bit counter
                self.high += HIGH_STEP
                self.words.append(0x8000 | self.high & 4095)
            self.words.append(0x8000 | high & 4095)
            self.high = high
        elif self.count % self.period == 0:
            self.words.append(0x8000 | high & 4095)
        if self.low is None or low != self.low or moved:
            self.words.append(0x6000 | low)
        if self.row is None or y != self.row:
            self.words.append(y)
        self.low, self.row = low, y
        if len(xs) == 1:
            self.words.append(0x2000 | p << 11 | xs[0])
        else:
            mask = sum(1 << (x - xs[0]) for x in xs)
            self.words += [0x3000 | p << 11 | xs[0], (0x4000 if mask >= 256 else 0x5000) | mask]
            self.vector_groups += 1
        self.count += 1
        self.groups += 1


def encode(t, x, y, p, fmt, vectors=False, high_period=64, first_time_high=0) -> np.ndarray:
    e = Encoder(fmt, vectors, high_period, first_time_high)
    for ev in zip(*(np.asarray(a, dtype=np.int64).tolist() for a in (t, x, y, p))):
        e.push(*ev)
    e.flush()
    return np.array(e.words, dtype='<u4' if fmt == 2 else '<u2')


# ---- streams ------------------------------------------------------------------------------------------------------------------------------
U = 1 << 12                                                      # one EVT3 TIME_HIGH unit in microseconds
PAUSES = [HIGH_STEP * U, HIGH_STEP * U + 1, (HIGH_STEP + 1) * U, 4097 * U, 5000 * U]


def _cols(ev):
    t, x, y, p = (np.array([e[i] for e in ev], dtype=np.int64) for i in range(4))
    return t, x, y, p


def hand_cases():
    """name -> (t, x, y, p): the cases the issue of the device encoder lists."""
    c = {'none': [], 'one': [(5, 3, 2, 1)]}
    for d in (1, 7, 8, 11, 12):
        c[f'pair_{d}'] = [(9, 10, 4, 1), (9, 10 + d, 4, 1)]
    c['descending'] = [(9, 20, 4, 1), (9, 19, 4, 1), (9, 18, 4, 1)]
    c['equal'] = [(9, 20, 4, 0), (9, 20, 4, 0), (9, 21, 4, 0)]
    c['polarity'] = [(9, 20, 4, 0), (9, 21, 4, 0), (9, 22, 4, 1), (9, 23, 4, 1), (9, 24, 4, 0)]
    c['row'] = [(7000, x, 100, 1) for x in range(304)]
    c['row_alternate'] = [(7000, x, 100, 0) for x in range(0, 304, 2)]
    for name, gap in (('1024', 1024 * U), ('1025', 1025 * U), ('5000', 5000 * U)):
        c[f'pause_{name}'] = [(100, 1, 1, 1), (100 + gap, 2, 1, 1), (100 + gap, 3, 1, 1), (101 + 2 * gap, 3, 1, 0)]
    c['across_2_24'] = [((1 << 24) - 3, 5, 5, 1), ((1 << 24) - 1, 6, 5, 1), (1 << 24, 7, 5, 1), ((1 << 24) + 4096, 8, 5, 1)]
    c['zero'] = [(0, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 1), (1, 0, 0, 0)]
    c['late'] = [((1 << 32) - 4097, 9, 9, 1), ((1 << 32) - 2, 9, 9, 1), ((1 << 32) - 1, 10, 9, 1), ((1 << 32) - 1, 11, 9, 1)]
    return {k: _cols(v) for k, v in c.items()}


def random_stream(rng, n, hw=(6, 40)):
    """About ``n`` events on a tiny sensor with few distinct times, so that vector runs are common: bursts of one row, time and polarity
    with mostly ascending columns; pauses of more than 1024 and more than 4096 TIME_HIGH units; a start beyond 2^24 us now and then."""
    H, W = hw
    ev = []
    now = int(rng.choice([0, 5, 1 << 24, (1 << 24) + 77]))
    while len(ev) < n:
        r = rng.rand()
        if r < 0.03:
            pause = int(rng.choice(PAUSES))
            if now + pause < (1 << 32) - (1 << 20):
                now += pause
        elif r < 0.5:
            now += int(rng.randint(0, 3))
        elif r < 0.6:
            now += int(rng.randint(1, 9000))
        k, row, pol = int(rng.randint(1, 14)), int(rng.randint(H)), int(rng.randint(2))
        xs = rng.randint(0, W, k)
        mode = rng.rand()
        if mode < 0.5:
            xs = np.unique(xs)                                   # strictly ascending
        elif mode < 0.7:
            xs = np.sort(xs)                                     # equal columns break a run
        for x in xs.tolist():
            ev.append((now, x, row if rng.rand() < 0.95 else int(rng.randint(H)), pol if rng.rand() < 0.95 else 1 - pol))
    return _cols(ev)
