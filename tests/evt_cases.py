"""Word lists that tests/test_evt_cpu.py (against the sequential decoder) and tests/test_evt_gpu.py (against the device decoder) share: the
hand-written cases with their events stated literally, and random streams that are rich in state words."""
import numpy as np

TH, TL, AY, AX, VB, V12, V8 = 0x8000, 0x6000, 0x0000, 0x2000, 0x3000, 0x4000, 0x5000
P1 = 0x800                                                       # polarity bit of ADDR_X / VECT_BASE_X

# (name, fmt, words, expected events (t, x, y, p), expected non-zero counters); tests/test_evt_gpu.py decodes the same lists on the device
HAND = [
    ('vect12_then_vect8_from_one_base', 3,
     [TH | 5, TL | 7, AY | 3, VB | P1 | 100, V12 | 0b100000000101, V8 | 0b10000001],
     [(7, 100, 3, 1), (7, 102, 3, 1), (7, 111, 3, 1), (7, 112, 3, 1), (7, 119, 3, 1)], {}),
    ('vector_before_any_base', 3,
     [TH | 1, TL | 0, AY | 9, V12 | 0b111, AX | 4, VB | 20, V8 | 0b1],
     [(0, 4, 9, 0), (0, 20, 9, 0)], dict(early_events=3)),
    ('event_before_the_first_time_low', 3,
     [TH | 2, AY | 1, AX | P1 | 8, TL | 50, AX | P1 | 9],
     [(50, 9, 1, 1)], dict(early_events=1)),
    ('time_high_4095_to_1_is_one_wrap', 3,
     [TH | 4095, TL | 10, AY | 0, AX | 1, TH | 1, TL | 20, AX | 2],
     [(10, 1, 0, 0), (2 * 4096 + 20, 2, 0, 0)], dict(wraps=1)),
    ('time_high_100_to_99_is_no_wrap_and_unsorted', 3,
     [TH | 90, TH | 100, TL | 5, AY | 2, AX | 1, TH | 99, AX | 2],
     [(10 * 4096 + 5, 1, 2, 0), (9 * 4096 + 5, 2, 2, 0)], {}),
    ('unknown_and_ignored_types', 3,
     [TH | 0, TL | 1, AY | 1, 0x1000, 0x7001, 0x9002, 0xA003, 0xB004, 0xC005, 0xD006, 0xE007, 0xF008, AX | 3],
     [(1, 3, 1, 0)], dict(ignored_words=4, unknown_words=5)),
    ('evt2_events_early_ignored_unknown', 2,
     [(0x1 << 28) | (5 << 22) | (7 << 11) | 9, (0x8 << 28) | 3, (0x0 << 28) | (5 << 22) | (7 << 11) | 9, (0xA << 28), (0xE << 28) | 1,
      (0xF << 28), (0x2 << 28), (0x8 << 28) | 4, (0x1 << 28) | (63 << 22) | (2047 << 11) | 2047],
     [(5, 7, 9, 0), (64 + 63, 2047, 2047, 1)], dict(early_events=1, ignored_words=3, unknown_words=1)),
]


def random_words(rng, n, fmt):
    if fmt == 2:
        kinds = rng.choice([0x0, 0x1, 0x8, 0x8, 0xA, 0x3], n)
        return (kinds.astype(np.int64) << 28) | rng.randint(0, 1 << 28, n)
    kinds = rng.choice([0x0, 0x2, 0x3, 0x4, 0x5, 0x6, 0x8, 0x8, 0x7, 0x1], n)
    pay = rng.randint(0, 4096, n)
    near = rng.rand(n) < 0.5                                      # TIME_HIGH values near both ends of the range: wraps and near-wraps
    pay = np.where((kinds == 0x8) & near, rng.choice([0, 1, 2047, 2048, 2049, 4094, 4095], n), pay)
    return (kinds.astype(np.int64) << 12) | pay
