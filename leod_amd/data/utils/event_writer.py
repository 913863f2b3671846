"""Event files written from records on the device: the way back of the ingestion.  ``EventFileWriter`` takes the 8-byte ``.dat`` records
of a recording chunk by chunk (as ``ops.decode_evt`` and the filter ops hand them on) and writes a Prophesee ``.dat`` file (the records are
the payload already) or a Metavision ``.raw`` file, EVT2 or EVT3, whose words ``ops.encode_evt`` (csrc/k_evtenc.hip) makes on the device
with the carried state.  The headers are those of ``dat_events.write_dat`` and ``raw_events.write_raw`` (``style='format'``, with
``% end``), which hold no clock: two runs write identical bytes.

No Metavision tool has read a file written here; the words are pinned against ``raw_events.encode_evt2`` / ``encode_evt3`` and against
this project's own decoder only."""
import os

import numpy as np

from leod_amd.data.utils import dat_events, raw_events

FORMATS = ('dat', 'evt2', 'evt3')
EVT_MAX_SIDE = 2048                                              # EVT words hold 11 bits of x and of y
SUFFIX = {'dat': '_td.dat', 'evt2': '.raw', 'evt3': '.raw'}      # <name> + this: what the ingestion looks for in a source directory


def check_format(fmt, height, width, vectors=False) -> None:
    """``ValueError`` for a format, a geometry or a vector option no file can be written with."""
    if fmt not in FORMATS:
        raise ValueError(f'write_events={fmt!r}: one of {FORMATS} expected')
    if vectors not in (False, True):
        raise ValueError(f'evt3_vectors={vectors!r}: True or False expected')
    if vectors and fmt != 'evt3':
        raise ValueError(f'evt3_vectors: only EVT3 has vector words, the format written is {fmt}')
    for name, v in (('height', height), ('width', width)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f'{name}={v!r}: a positive integer expected')
    if fmt != 'dat' and (height > EVT_MAX_SIDE or width > EVT_MAX_SIDE):
        raise ValueError(f'a {width}x{height} geometry does not fit {fmt.upper()}, whose words hold 11 bits of x and of y '
                         f'(at most {EVT_MAX_SIDE}x{EVT_MAX_SIDE}); write dat')


class EventFileWriter:
    """``append`` takes the records of a chunk on the device (uint8 [n, 8] or [n * 8], stream order, t non-decreasing), encodes them,
    copies the bytes to the host and appends them to ``fn + '.tmp'``; ``close`` writes what the encoder still holds (``final=True``) and
    renames the file; ``abort`` removes the temporary file (the contract of ``packed.PackedWriter``).  ``events``, ``words`` (EVT) and
    ``payload_bytes`` count what was written."""

    def __init__(self, fn: str, fmt: str, height: int, width: int, vectors: bool = False):
        check_format(fmt, height, width, vectors)
        self.fn, self.fmt, self.height, self.width, self.vectors = fn, fmt, int(height), int(width), bool(vectors)
        self.events, self.words, self.payload_bytes, self._state, self._device = 0, 0, 0, None, None
        if fmt == 'dat':
            dat_events.write_dat(fn + '.tmp', np.zeros((0, 2), dtype='<u4'), self.height, self.width)
        else:
            raw_events.write_raw(fn + '.tmp', np.zeros((0,), dtype=raw_events.WORD_DTYPE[fmt]), fmt, self.height, self.width)
        self._f = open(fn + '.tmp', 'ab')

    def append_bytes(self, payload) -> None:
        """Payload bytes that are encoded already (whole records / words), e.g. those of a host encoder."""
        data = memoryview(np.ascontiguousarray(payload)).cast('B')
        unit = dat_events.EVENT_SIZE if self.fmt == 'dat' else raw_events.WORD_BYTES[self.fmt]
        if len(data) % unit:
            raise ValueError(f'{self.fn}: {len(data)} bytes are no whole number of {unit}-byte {"records" if self.fmt == "dat" else "words"}')
        self._f.write(data)
        self.payload_bytes += len(data)
        if self.fmt != 'dat':
            self.words += len(data) // unit

    def _encode(self, records, final: bool) -> None:
        from leod_amd import ops
        words, self._state = ops.encode_evt(records, self.fmt, self._state, final=final, vectors=self.vectors)
        self.append_bytes(words.cpu().numpy())

    def append(self, records) -> None:
        records = records.reshape(-1)
        if records.numel() % dat_events.EVENT_SIZE:
            raise ValueError(f'{self.fn}: {records.numel()} bytes are no whole number of {dat_events.EVENT_SIZE}-byte events')
        self.events += records.numel() // dat_events.EVENT_SIZE
        if self.fmt == 'dat':
            self.append_bytes(records.cpu().numpy())
        else:
            self._device = records.device
            self._encode(records, False)

    def close(self) -> None:
        if self.fmt != 'dat' and (self._state is not None or self.payload_bytes == 0):   # fed by append_bytes alone: nothing is held
            import torch
            device = self._device if self._device is not None else torch.device('cuda', torch.cuda.current_device())
            self._encode(torch.empty((0,), dtype=torch.uint8, device=device), True)     # a recording of no events is its opening word
        self._f.close()
        os.replace(self.fn + '.tmp', self.fn)

    def abort(self) -> None:
        self._f.close()
        if os.path.exists(self.fn + '.tmp'):
            os.remove(self.fn + '.tmp')
