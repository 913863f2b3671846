"""Filter survey: what every noise filter of the ingestion would remove from a recording, for a whole list of thresholds, from ONE pass
over its events (``ops.survey_events``, csrc/k_survey.hip; the definitions and identities: DESIGN.md section 1).  It writes nothing into
a dataset tree and changes nothing in the ingestion: it is the tool to choose ``--denoise-us``, ``--trail-us``, ``--stc-us`` /
``--stc-cut-trail``, ``--anti-flicker`` / ``--flicker-lock`` and ``--hot-rate`` with.

Every ``<name>_td.dat`` and ``<name>.raw`` of SRC is read through the ingestion's chunk reader, at sensor resolution (Gen4 too), and one
JSON object per recording is printed: the head counters, the histograms, the response curves (``event_filter.survey_responses``) and,
with ``--hot-rates``, the number of pixels ``event_filter.hot_pixel_mask`` would mask at each rate.

EACH CURVE IS FOR THAT FILTER APPLIED ALONE TO THE UNFILTERED STREAM (behind the bounds and ``--pixel-mask``).  In a combined ingestion
the per-pixel filters run first and the activity filter (``--denoise-us``) sees only what they keep, so its count there differs.

    python -m leod_amd.data.survey SRC --dataset gen1|gen4 [--edges-us E ...] [--anti-flicker FMIN:FMAX] [--pixel-mask FILE.npy]
                                   [--hot-rates HZ ...] [--out REPORT.json] [--sensor WxH]

``--sensor WxH`` surveys a recording of another sensor (a VGA camera, say) at its own resolution; a size in the file's header must agree
with it.  The survey applies no sensor fit (``--fit`` of the ingestion): the ingestion's filters run before the fit, at this geometry.
"""
import argparse
import glob
import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from leod_amd.data.ingest import RAW_CHUNK_BYTES, SENSOR_HW, _RecordChunks, _dataset_type, _order_error, parse_sensor
from leod_amd.data.utils import dat_events, event_filter as ef

# 100 us to 100 ms: the 1-2-5 steps of each decade with 3 and 7 between them, 16 edges
DEFAULT_EDGES_US = (100, 200, 300, 500, 700, 1_000, 2_000, 3_000, 5_000, 7_000, 10_000, 20_000, 30_000, 50_000, 70_000, 100_000)
MAX_EDGES = 64
NOTE = ('Each curve counts the events that ONE filter removes when it is applied alone to the unfiltered stream (behind the sensor '
        'bounds and the pixel mask). In a combined ingestion the per-pixel filters run first and the activity filter (denoise) sees '
        'only what they keep.')


def check_edges(edges_us) -> List[int]:
    """``ValueError`` unless ``edges_us`` is a strictly increasing list of 1 to 64 whole microseconds in [0, 2^31); -> the list."""
    try:
        edges = list(edges_us)
    except TypeError:
        raise ValueError(f'edges_us={edges_us!r}: a list of integers expected') from None
    if not 1 <= len(edges) <= MAX_EDGES:
        raise ValueError(f'edges_us: {len(edges)} edges; 1 to {MAX_EDGES} expected')
    for e in edges:
        if isinstance(e, (bool, float)) or not isinstance(e, (int, np.integer)) or not 0 <= int(e) < 2 ** 31:
            raise ValueError(f'edges_us: {e!r}; whole microseconds in [0, 2^31) expected')
    edges = [int(e) for e in edges]
    for a, b in zip(edges[:-1], edges[1:]):
        if not a < b:
            raise ValueError(f'edges_us: {a} is followed by {b}; a strictly increasing list expected')
    return edges


def check_survey_options(dataset_type, edges_us=None, anti_flicker=None, pixel_mask=None, hot_rates=None, sensor_hw=None) -> Dict:
    """The options of a call, checked on the host before anything is opened -> dict(edges, band, mask, hot_rates): ``edges_us`` None is
    ``DEFAULT_EDGES_US``; ``anti_flicker`` 'FMIN:FMAX' or (fmin, fmax) -> ``band`` (p_min_us, p_max_us) or None; ``pixel_mask`` a ``.npy``
    file name or an array at the dataset's sensor resolution; ``hot_rates`` non-negative integer rates in events per second;
    ``sensor_hw`` ('WxH' or (height, width); None: the dataset's) -> ``sensor`` (height, width), the resolution of the survey and of the mask (a key only where it is given)."""
    sensor = SENSOR_HW[_dataset_type(dataset_type)] if sensor_hw is None else parse_sensor(sensor_hw)
    edges = check_edges(DEFAULT_EDGES_US if edges_us is None else edges_us)
    band = None if anti_flicker is None else ef.flicker_band(anti_flicker)
    mask = None
    if pixel_mask is not None:
        mask = ef.read_pixel_mask(pixel_mask, sensor) if isinstance(pixel_mask, (str, os.PathLike)) else ef.check_pixel_mask(pixel_mask, sensor)
    rates = []
    for r in (hot_rates or ()):
        if isinstance(r, (bool, float)) or not isinstance(r, (int, np.integer)) or int(r) < 0:
            raise ValueError(f'hot_rates: {r!r}; non-negative integer rates in events per second expected')
        rates.append(int(r))
    opt = dict(edges=edges, band=band, mask=mask, hot_rates=rates)
    if sensor_hw is not None:
        opt['sensor'] = tuple(sensor)
    return opt


def _open_payload(ev_fn: str):
    """(header, payload bytes, encoding) of a ``.dat`` or ``.raw`` file, as the streaming ingestion opens them."""
    if ev_fn.lower().endswith('.raw'):
        from leod_amd.data.utils import raw_events
        hdr, payload = raw_events.open_words(ev_fn)
        return hdr, payload, hdr.encoding
    hdr, records = dat_events.open_records(ev_fn)
    return hdr, records.view(np.uint8).reshape(-1), 'dat'


def _record_chunks(payload, encoding, raw_chunk_bytes, what):
    """The ingestion's chunk reader on the current device."""
    import torch
    device = torch.device('cuda', torch.cuda.current_device())
    return _RecordChunks(payload, encoding, raw_chunk_bytes, device, what)


def survey_recording(ev_fn: str, dataset_type, edges_us=None, anti_flicker=None, pixel_mask=None, hot_rates: Optional[Sequence[int]] = None,
                     raw_chunk_bytes: Optional[int] = None, sensor_hw=None) -> Dict:
    """One recording -> its report (plain Python numbers and lists, ready for JSON): recording, sensor, edges_us, band_us, the head
    counters of the survey, ``histograms`` (nb, same, sec_on, sec_off, period, run), ``removed`` (``event_filter.survey_responses``:
    denoise, trail, stc, stc_cut_trail per edge; flicker_by_lock, entry L - 1 for lock L = 1 .. 255), with ``hot_rates`` ``hot_pixels``
    (rate -> pixels ``hot_pixel_mask`` masks, from ``ops.event_pixel_counts`` over the same chunks) and ``note``.  ``sensor_hw``: the
    recording's own sensor where it is not the dataset's; a size in the header that differs from it is a ``ValueError``."""
    import torch
    from leod_amd import ops
    dataset_type = _dataset_type(dataset_type)
    opt = check_survey_options(dataset_type, edges_us, anti_flicker, pixel_mask, hot_rates, sensor_hw)
    height, width = opt.get('sensor', SENSOR_HW[dataset_type])
    hdr, payload, encoding = _open_payload(ev_fn)
    names = ('height', 'width') if ev_fn.lower().endswith('.raw') else ('Height', 'Width')
    for name, got, want in zip(names, (hdr.height, hdr.width), (height, width)):
        if got is not None and got != want:
            if sensor_hw is not None:
                raise ValueError(f'{ev_fn}: header says {name} {got}, the sensor given has {want}')
            raise ValueError(f'{ev_fn}: header says {name} {got}, a {dataset_type.name} recording has {want}')
    edges, band = opt['edges'], opt['band']
    state, counts, mask = None, None, None
    for rec in _record_chunks(payload, encoding, RAW_CHUNK_BYTES if raw_chunk_bytes is None else raw_chunk_bytes, ev_fn):
        if rec.shape[0] == 0:
            continue
        if opt['mask'] is not None and mask is None:
            mask = torch.from_numpy(np.ascontiguousarray(opt['mask'], dtype=np.uint8)).to(rec.device)
        try:
            state = ops.survey_events(rec, height, width, edges, flicker=band, state=state, pixel_mask=mask)
        except ops.EventOrderError as e:
            raise _order_error(ev_fn, e.t_before, e.t_at) from None
        if opt['hot_rates']:
            counts, _ = ops.event_pixel_counts(rec, height, width, counts)
    K = len(edges)
    if state is None:                                            # a recording of zero events
        c = dict(seen=0, candidates=0, outside=0, masked=0, t_first=-1, t_last=-1, nb=np.zeros(K + 2, np.int64),
                 same=np.zeros(K + 1, np.int64), sec_on=np.zeros(K + 1, np.int64), sec_off=np.zeros(K + 1, np.int64),
                 period=np.zeros(K + 1, np.int64), run=np.zeros(256, np.int64))
    else:
        c = ops.survey_counters(state, K)
    resp = ef.survey_responses(c, edges)
    rep = dict(recording=ev_fn, sensor=[height, width], edges_us=edges, band_us=None if band is None else list(band),
               masked_pixels=int(np.count_nonzero(opt['mask'])) if opt['mask'] is not None else 0)
    rep.update({k: int(c[k]) for k in ('seen', 'candidates', 'outside', 'masked', 't_first', 't_last')})
    rep['histograms'] = {k: [int(v) for v in c[k]] for k in ('nb', 'same', 'sec_on', 'sec_off', 'period', 'run')}
    rep['removed'] = {k: [int(v) for v in resp[k]] for k in ('denoise', 'trail', 'stc', 'stc_cut_trail')}
    rep['removed']['flicker_by_lock'] = [int(v) for v in resp['flicker'][1:]] if band is not None else None
    if opt['hot_rates']:
        duration = max(rep['t_last'] - rep['t_first'], 1)        # as the ingestion's --hot-rate takes it
        per_pixel = np.zeros((height, width), np.int64) if counts is None else counts.cpu().numpy()
        rep['hot_pixels'] = {str(r): int(np.count_nonzero(ef.hot_pixel_mask(per_pixel, duration, r))) for r in opt['hot_rates']}
    rep['note'] = NOTE
    return rep


def survey_split(src_dir: str, dataset_type, verbose: bool = False, **kw) -> List[Dict]:
    """Every ``<name>_td.dat`` and ``<name>.raw`` of ``src_dir`` -> the reports of ``survey_recording``, in file-name order."""
    reports = []
    for fn in sorted(glob.glob(os.path.join(src_dir, '*_td.dat')) + glob.glob(os.path.join(src_dir, '*.raw'))):
        rep = survey_recording(fn, dataset_type, **kw)
        if verbose:
            print(json.dumps(rep), flush=True)
        reports.append(rep)
    return reports


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog='python -m leod_amd.data.survey', description=__doc__.split('\n\n')[0], epilog=NOTE)
    ap.add_argument('src', help='directory of *_td.dat / *.raw recordings')
    ap.add_argument('--dataset', required=True, choices=['gen1', 'gen4'])
    ap.add_argument('--edges-us', type=int, nargs='+', default=None, metavar='E',
                    help=f'1 to {MAX_EDGES} strictly increasing thresholds in microseconds (default: {" ".join(map(str, DEFAULT_EDGES_US))})')
    ap.add_argument('--anti-flicker', default=None, metavar='FMIN:FMAX',
                    help='the band of the anti-flicker filter in integer Hz: adds the events removed at every --flicker-lock 1 .. 255')
    ap.add_argument('--pixel-mask', default=None, metavar='FILE.npy',
                    help='uint8 / bool array [H, W] at sensor resolution; the events of its non-zero pixels are counted as masked')
    ap.add_argument('--hot-rates', type=int, nargs='+', default=None, metavar='HZ',
                    help='also count, per rate, the pixels --hot-rate HZ would mask')
    ap.add_argument('--sensor', default=None, metavar='WxH', help="the recording's own sensor size, e.g. 640x480, where it is not the dataset's")
    ap.add_argument('--out', default=None, metavar='REPORT.json', help='also write the list of reports to this file')
    args = ap.parse_args(argv)
    kw = dict(edges_us=args.edges_us, anti_flicker=args.anti_flicker, pixel_mask=args.pixel_mask, hot_rates=args.hot_rates,
              sensor_hw=args.sensor)
    try:
        check_survey_options(args.dataset, **kw)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    reports = survey_split(args.src, args.dataset, verbose=True, **kw)
    if not reports:
        ap.error(f'no *_td.dat or *.raw under {args.src}')
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(reports, f, indent=1)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
