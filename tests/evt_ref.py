"""The sequential EVT2 / EVT3 decoder the tests hold ``ops.decode_evt`` and the encoders against: one word at a time, a state that can be
carried from one ``feed`` to the next, written from the rules of DESIGN.md section 1 and independently of ``raw_events.decode``.

``Decoder(fmt).feed(words)`` -> records [n, 2] u32 as a .dat file holds them (t reduced to 32 bits; x | y << 14 | p << 28);
``.state()`` -> the 16 integers of the device state block (include/leod_hip.h), ``.counters()`` -> what ``ops.evt_state_counters`` gives."""
import numpy as np

IGNORED = {2: (0xA, 0xE, 0xF), 3: (0x7, 0xA, 0xE, 0xF)}


class Decoder:
    def __init__(self, fmt: int):
        assert fmt in (2, 3)
        self.fmt = fmt
        self.have_high = self.have_low = self.have_y = self.have_base = False
        self.high = self.wraps = self.low = self.y = self.base = self.vpol = self.time_base = 0
        self.events = self.early = self.ignored = self.unknown = self.overflow = self.last_chunk = 0

    # -- one event -----------------------------------------------------------------------------------------------------------------
    def _event(self, out, t_abs, x, y, p):
        t = t_abs - self.time_base
        if t < 0 or t >= 2 ** 32:
            self.overflow = 1
        out.append((t & 0xffffffff, (x & 0x3fff) | (y << 14) | (p << 28)))

    def _word2(self, w, out):
        kind = w >> 28
        if kind == 0x8:
            self.high = w & 0x0fffffff
            if not self.have_high:
                self.have_high, self.time_base = True, self.high << 6
        elif kind in (0, 1):
            if self.have_high:
                self._event(out, (self.high << 6) | ((w >> 22) & 0x3f), (w >> 11) & 0x7ff, w & 0x7ff, kind)
            else:
                self.early += 1
        elif kind in IGNORED[2]:
            self.ignored += 1
        else:
            self.unknown += 1

    def _word3(self, w, out):
        kind, v = w >> 12, w & 0xfff
        if kind == 0x8:
            if not self.have_high:
                self.have_high, self.time_base = True, v << 12
            elif self.high - v >= 2048:
                self.wraps += 1
            self.high = v
        elif kind == 0x6:
            self.low, self.have_low = v, True
        elif kind == 0x0:
            self.y, self.have_y = v & 0x7ff, True
        elif kind == 0x3:
            self.base, self.vpol, self.have_base = v & 0x7ff, v >> 11, True
        elif kind in (0x2, 0x4, 0x5):
            timed = self.have_high and self.have_low and self.have_y
            t_abs = ((self.wraps * 4096 + self.high) << 12) | self.low
            if kind == 0x2:
                if timed:
                    self._event(out, t_abs, v & 0x7ff, self.y, v >> 11)
                else:
                    self.early += 1
                return
            width = 12 if kind == 0x4 else 8
            for i in range(width):
                if v >> i & 1:
                    if timed and self.have_base:
                        self._event(out, t_abs, self.base + i, self.y, self.vpol)
                    else:
                        self.early += 1
            self.base += width                                    # without a base this is never read: VECT_BASE_X overwrites it
        elif kind in IGNORED[3]:
            self.ignored += 1
        else:
            self.unknown += 1

    def feed(self, words) -> np.ndarray:
        out = []
        step = self._word3 if self.fmt == 3 else self._word2
        for w in np.asarray(words, dtype=np.int64).reshape(-1).tolist():
            step(w, out)
        self.events += len(out)
        self.last_chunk = len(out)
        return np.array(out, dtype=np.int64).reshape(-1, 2).astype('<u4')

    def state(self):
        valid = self.have_high * 1 + self.have_low * 2 + self.have_y * 4 + self.have_base * 8
        return [valid, self.high, self.wraps, self.low, self.y, self.base & 0xffffffff, self.vpol, self.time_base, self.events, self.early,
                self.ignored, self.unknown, self.overflow, self.fmt, self.last_chunk, 0]

    def counters(self):
        return dict(events=self.events, early_events=self.early, ignored_words=self.ignored, unknown_words=self.unknown,
                    overflow=self.overflow, wraps=self.wraps)


def decode(words, fmt):
    """words -> (t, x, y, p) int64 of the records + the decoder (its counters / state)."""
    d = Decoder(fmt)
    r = d.feed(words).astype(np.int64)
    return (r[:, 0], r[:, 1] & 0x3fff, (r[:, 1] >> 14) & 0x3fff, (r[:, 1] >> 28) & 1), d


def as_bytes(words, fmt) -> np.ndarray:
    return np.asarray(words, dtype='<u2' if fmt == 3 else '<u4').view(np.uint8).reshape(-1)
