"""Where the time of a JPEG decode goes (DESIGN.md 3.4 "JPEG decoder"): hipops.jpeg_decode -- host parse, upload of the file's bytes, the
device stages, the status read -- against what it replaces, PIL.Image.open(...).convert('RGB') plus the upload of its pixels, on the same
bytes.

Cases: a synthetic 3000 x 4000 photograph and a 512 x 512 one (band-limited noise plus +-20 uniform noise, the content of the tests'
`textured`), written by PIL as 4:2:0 quality 92 without restart markers.  Per case the median and range of 7 windows after a warm-up: the whole
GPU call (host clock around a synchronise), the device work alone (events), every stage alone (events; EG3D_JPEGDEC_STAGE_*), the parse and
the upload, the PIL decode and the upload of its pixels; the synchronisation rounds and lanes at several subsequence sizes.

  python tools/time_jpeg_decode.py [--windows 7] [--sizes 3000x4000,512x512] [--out result.json]

--batch: hipops.jpeg_decode_batch instead -- N photographs of different content (seeds 0 .. N - 1) in one call, N in 1, 4, 16, 64 at 512 x 512
and 1, 4 at 3000 x 4000 (--batch-sizes) -- beside N single jpeg_decode calls and beside the PIL decode + upload of the pixels per file, all in
one session: the whole call and the device work alone, in total and per frame, and every stage of the batch alone.

  python tools/time_jpeg_decode.py --batch [--windows 7] [--batch-sizes 512x512:1,4,16,64;3000x4000:1,4] [--out result.json]"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from inv3d_amd import _lib as L, hipops as H, video as V  # noqa: E402


def stat(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def device_ms(fn, windows):
    out = []
    for _ in range(windows + 1):                                              # the first window warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return stat(out[1:])


def host_ms(fn, windows):
    out = []
    for i in range(windows + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return stat(out[1:])


def photograph(width, height, seed=0):
    """uint8 [H,W,3]: noise at 1/16 resolution blown up bicubically (the smooth part), plus +-20 uniform noise"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(1, 3, height // 16 + 2, width // 16 + 2, generator=g)
    smooth = torch.nn.functional.interpolate(low, size=(height, width), mode='bicubic', align_corners=False)[0]
    smooth = (smooth - smooth.min()) / (smooth.max() - smooth.min()) * 255
    noise = torch.randint(-20, 21, smooth.shape, generator=g)
    return (smooth + noise).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def time_case(width, height, windows, subseqs):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(photograph(width, height)).save(buf, 'JPEG', quality=92, subsampling=2)
    data = buf.getvalue()
    plan = V.jpeg_scan_plan(data)
    res = dict(case=f'{width}x{height}', file_bytes=len(data), scan_bytes=plan.scan_end - plan.scan_start, pixels=width * height)

    def pil():
        with Image.open(io.BytesIO(data)) as im:
            return np.array(im.convert('RGB'), dtype=np.uint8)
    want = pil()
    stats = {}
    got = H.jpeg_decode(data, stats=stats)
    res['equal_to_pil'] = bool(np.array_equal(got.cpu().numpy(), want))
    res['gpu_call_ms'] = host_ms(lambda: H.jpeg_decode(data), windows)
    res['pil_decode_ms'] = host_ms(pil, windows)
    res['pil_decode_and_upload_ms'] = host_ms(lambda: torch.from_numpy(pil()).cuda(), windows)
    res['parse_ms'] = host_ms(lambda: V.jpeg_scan_plan(data), windows)
    p, keep, out, result = H._jpegdec_begin(data, 128)
    res['parse_upload_allocate_ms'] = host_ms(lambda: H._jpegdec_begin(data, 128), windows)
    lib = L.lib()

    def run(stages):
        p.stages = stages
        L.check(lib.eg3d_jpegdec_decode(C.byref(p), L.stream_ptr()), 'jpegdec_decode')
    run(0)
    res['device_ms'] = device_ms(lambda: run(0), windows)
    res['stage_ms'] = {name: device_ms(lambda: run(bit), windows) for name, bit in L.JPEGDEC_STAGES.items()}
    run(0)
    assert result.tolist()[0] == 0 and bool((out == got).all())
    res['by_subseq_bytes'] = {}
    for B in subseqs:
        st = {}
        H.jpeg_decode(data, subseq_bytes=B, stats=st)
        pb, keepb, _, _ = H._jpegdec_begin(data, B)

        def runb(stages):
            pb.stages = stages
            L.check(lib.eg3d_jpegdec_decode(C.byref(pb), L.stream_ptr()), 'jpegdec_decode')
        runb(0)
        res['by_subseq_bytes'][B] = dict(lanes=st['lanes'], rounds_workgroup=st['rounds_workgroup'], rounds_across=st['rounds_across'],
                                         device_ms=device_ms(lambda: runb(0), windows), sync_ms=device_ms(lambda: runb(2), windows),
                                         write_ms=device_ms(lambda: runb(4), windows))
        del keepb
    del keep
    return res


def time_batch(width, height, ns, windows):
    from PIL import Image
    files = []
    for seed in range(max(ns)):
        buf = io.BytesIO()
        Image.fromarray(photograph(width, height, seed)).save(buf, 'JPEG', quality=92, subsampling=2)
        files.append(buf.getvalue())

    def pil(data):
        with Image.open(io.BytesIO(data)) as im:
            return np.array(im.convert('RGB'), dtype=np.uint8)
    lib = L.lib()
    res = dict(case=f'{width}x{height}', file_bytes=[len(f) for f in files[:4]], by_n={})
    for n in ns:
        fs = files[:n]
        got = H.jpeg_decode_batch(fs)
        r = dict(equal_to_pil=all(bool(np.array_equal(g.cpu().numpy(), pil(f))) for g, f in zip(got[:4], fs)))
        r['batch_call_ms'] = host_ms(lambda: H.jpeg_decode_batch(fs), windows)
        r['single_calls_ms'] = host_ms(lambda: [H.jpeg_decode(f) for f in fs], windows)
        r['pil_decode_and_upload_ms'] = host_ms(lambda: [torch.from_numpy(pil(f)).cuda() for f in fs], windows)
        plans = [V.jpeg_scan_plan(f) for f in fs]
        p, keep, outs, result = H._jpegdec_batch_begin(fs, plans, 128)

        def run(stages):
            p.stages = stages
            L.check(lib.eg3d_jpegdec_batch_decode(C.byref(p), L.stream_ptr()), 'jpegdec_batch_decode')
        run(0)
        r['batch_device_ms'] = device_ms(lambda: run(0), windows)
        r['batch_stage_ms'] = {name: device_ms(lambda: run(bit), windows) for name, bit in L.JPEGDEC_STAGES.items()}
        run(0)
        assert all(row[0] == 0 for row in result.tolist()) and all(bool((o == g).all()) for o, g in zip(outs, got))
        del keep
        singles = [H._jpegdec_begin(f, 128) for f in fs]

        def run_singles():
            for q, _, _, _ in singles:
                L.check(lib.eg3d_jpegdec_decode(C.byref(q), L.stream_ptr()), 'jpegdec_decode')
        run_singles()
        r['single_device_ms'] = device_ms(run_singles, windows)
        del singles
        r['per_frame_ms'] = {k: round(r[k]['median'] / n, 4) for k in ('batch_call_ms', 'single_calls_ms', 'pil_decode_and_upload_ms', 'batch_device_ms',
                                                                        'single_device_ms')}
        res['by_n'][n] = r
        print(json.dumps({'case': res['case'], 'n': n, **r}), flush=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--sizes', default='3000x4000,512x512', help='width x height, comma-separated')
    ap.add_argument('--subseq', default='32,64,128,256,512')
    ap.add_argument('--out', default=None)
    ap.add_argument('--batch', action='store_true', help='time hipops.jpeg_decode_batch beside single calls and PIL')
    ap.add_argument('--batch-sizes', default='512x512:1,4,16,64;3000x4000:1,4', help='width x height : batch sizes, semicolon-separated')
    a = ap.parse_args(argv)
    out = dict(device=torch.cuda.get_device_name(0), cases=[])
    for item in a.batch_sizes.split(';') if a.batch else ():
        size, ns = item.split(':')
        w, h = (int(v) for v in size.split('x'))
        out['cases'].append(time_batch(w, h, [int(v) for v in ns.split(',')], a.windows))
    for size in () if a.batch else a.sizes.split(','):
        w, h = (int(v) for v in size.split('x'))
        out['cases'].append(time_case(w, h, a.windows, [int(v) for v in a.subseq.split(',')]))
        print(json.dumps(out['cases'][-1]))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == '__main__':
    main()
