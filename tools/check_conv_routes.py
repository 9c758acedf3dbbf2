"""Check tests/golden/conv_routes.json against the launches a source tree really made (no GPU needed: it reads two JSON files).

    python tools/check_conv_routes.py tests/golden/conv_routes.json LAUNCHES.json

LAUNCHES.json: {"c2": [...], "c2n8": [...], "phase_b": [...]} -- per case the launches of a few EAGER steps under hipops.LaunchProfiler(keep_meta=True),
in order, each {"key": [kernel id, precision id], "meta": {...}} (c2: latent projection at one image, frozen weights; c2n8: eight images; phase_b:
pivotal tuning, trainable weights).  For every layer of the golden table and each of the three cases, the forward and the data-gradient launch the
table names must be among the recorded ones: kernel id, operand geometry, epilogue, patch rows, split factor and strides.

What it cannot see: a profiler record carries no layer name, so a route is matched by its signature (kernel id + the fields above), and layers or
passes with the same signature (the data gradients of two 512-channel layers on the same grid) are told apart only by COUNT: the recorded launches of
a signature must be a whole multiple of the golden routes that share it, and that multiple -- the number of recorded steps -- must be the same for
every signature of a case, so a doubled or dropped launch shows.  Launches of other operators (toRGB, loss networks) whose signature coincides with
a golden route would show as a COUNT failure, to be read by hand.  Weight-gradient launches carry no profiler record.
The kernel ids below are copies of hipops.*_CONFIG so that this file runs without the package."""
import json
import sys

STORE, ATOMIC, FWD, BWD = 0, 1, 2, 3
IGEMM, V2, UP2, S2ADJ, V2H, V3, WS, V2RGB = {0, 1, 2, 3, 4}, 5, 6, 7, 8, 11, 12, 13
CASES = {'c2': 'N1 frozen f16x3', 'c2n8': 'N8 frozen f16x3', 'phase_b': 'N1 trainable f16x3'}


def expected(geom, N, row):
    """[(pass, kernel ids, required meta fields)] for one golden row."""
    Ci, Co, Hi, Wi, up = (geom[k] for k in ('Ci', 'Co', 'Hi', 'Wi', 'up'))
    Hz, Wz = (Hi, Wi) if up == 1 else (2 * Hi + 1, 2 * Wi + 1)
    f, d = row['forward'], row['dgrad']
    fm = dict(N=N, Ck=Ci, Nc=Co, Ho=Hz, Wo=Wz)
    fwd = {'v2': ({V2, V2RGB} if f['rows'] == 8 else {V2H}, dict(fm, epi=FWD, patch_rows=f['rows'], out_stride=1)),
           'v3': ({V3}, dict(fm, epi=FWD, patch_rows=(f['v3'] or [0, 0])[0], ksplit=(f['v3'] or [0, 0])[1])),
           'up2': ({UP2}, dict(fm, Hi=Hi, Wi=Wi, epi=ATOMIC if f['ksplit'] > 1 else STORE, ksplit=f['ksplit'], out_stride=2)),
           'ws': ({WS}, dict(fm, in_stride=1, out_stride=1)), 'ws_up': ({WS}, dict(fm, Hi=Hi, Wi=Wi, out_stride=2)),
           'igemm': (IGEMM, dict(fm, epi=FWD, ksplit=1, out_stride=1)), 'igemm_up': (IGEMM, dict(fm, epi=STORE, ksplit=1, out_stride=up)),
           'igemm_splitk': (IGEMM, dict(fm, epi=ATOMIC, ksplit=f['ksplit'], out_stride=up))}[f['form']]
    dm = dict(N=N, Ck=Co, Nc=Ci, Ho=Hi, Wo=Wi)
    bwd = {'v2': ({V2} if d['rows'] == 8 else {V2H}, dict(dm, epi=BWD, patch_rows=d['rows'], in_stride=1)),
           'v3': ({V3}, dict(dm, epi=BWD, patch_rows=(d['v3'] or [0, 0])[0], ksplit=(d['v3'] or [0, 0])[1], in_stride=1)),
           's2adj': ({S2ADJ}, dict(dm, epi=BWD, in_stride=2)), 'v3_s2adj': ({V3}, dict(dm, epi=BWD, in_stride=2)),
           'ws': ({WS}, dict(dm, in_stride=1)), 'ws_s2': ({WS}, dict(dm, in_stride=2)),
           'igemm': (IGEMM, dict(dm, epi=BWD, ksplit=1, in_stride=up)),
           'igemm_splitk': (IGEMM, dict(dm, epi=ATOMIC, ksplit=d['ksplit'], in_stride=up))}[d['form']]
    return [('forward', f['form']) + fwd, ('dgrad', d['form']) + bwd]


def main(golden_path, launches_path):
    golden, launches = json.load(open(golden_path)), json.load(open(launches_path))
    bad = checked = 0
    for case, key in CASES.items():
        recs = launches[case]
        N = int(key.split()[0][1:])
        sigs = {}           # signature -> the golden routes that share it
        for name, layer in golden.items():
            for which, form, ids, want in expected(layer['geometry'], N, layer['routes'][key]):
                sigs.setdefault((tuple(sorted(ids)), tuple(sorted(want.items()))), []).append(f'{name} {which} {form}')
        steps = set()
        for (ids, want), routes in sigs.items():
            hits = sum(1 for r in recs if r['key'][0] in ids and all(r['meta'].get(k) == v for k, v in want))
            checked += len(routes)
            if not hits or hits % len(routes):
                bad += len(routes)
                print(f'{"MISSING" if not hits else "COUNT"} {case} {routes}: {hits} recorded launches of kernel ids {list(ids)} with {dict(want)}')
            else:
                steps.add(hits // len(routes))
        if len(steps) > 1:
            bad += 1
            print(f'COUNT {case}: routes recorded {sorted(steps)} times each -- a launch was doubled or dropped')
    print(f'{checked - bad} of {checked} golden routes found among the recorded launches')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
