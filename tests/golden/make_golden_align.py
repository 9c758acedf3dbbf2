#!/usr/bin/env python3
"""Face-alignment fixture generator (tests/golden/align.npz).  Runs on the CPU of a development machine with a checkout of the reference
(cvlab-kaist/3DGAN-Inversion), Pillow and scipy:

    python tests/golden/make_golden_align.py REFERENCE_ROOT

Loads the reference's utils/alignment.py with three changes -- a stub `dlib` module in sys.modules (the module imports it at the top; nothing
of it is called), PIL.Image.ANTIALIAS = PIL.Image.LANCZOS (the alias newer Pillow versions dropped), get_landmark replaced by a function that
returns the case's landmarks -- and runs its own align_face on seeded synthetic photographs (smooth colour fields plus noise) written as PNG
to a temporary directory.  Per case the fixture records the input image, the landmarks, output_size, the returned image and which branches
ran (shrink factor, crop, pad); the generator asserts that every branch combination the tests need occurs."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import PIL.Image

HERE = os.path.dirname(os.path.abspath(__file__))


def photo(h, w, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    ph = rs.uniform(0, 6.28, 6)
    f = rs.uniform(0.02, 0.09, 6)
    img = np.stack([130 + 70 * np.sin(xx * f[0] + ph[0]) * np.cos(yy * f[1] + ph[1]),
                    120 + 60 * np.sin(xx * f[2] + yy * f[3] + ph[2]),
                    110 + 80 * np.cos(yy * f[4] + ph[3]) * np.sin((xx - yy) * f[5] + ph[4])], -1)
    img = img + rs.normal(0.0, 6.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def landmarks(eye_left, eye_right, mouth, seed):
    """68 x 2 points: the six of each eye scattered about its centre (their mean is exactly the centre), mouth corners about `mouth`; the rest
    (never read by align_face) somewhere in between."""
    rs = np.random.RandomState(seed)
    lm = np.zeros((68, 2), np.float64)
    lm[:] = np.asarray(mouth) + rs.uniform(-5, 5, (68, 2))
    for sl, c in ((slice(36, 42), eye_left), (slice(42, 48), eye_right)):
        d = rs.uniform(-2, 2, (6, 2))
        lm[sl] = np.asarray(c) + d - d.mean(0)
    half = np.asarray([rs.uniform(4, 7), rs.uniform(-1, 1)])
    lm[48], lm[54] = np.asarray(mouth) - half, np.asarray(mouth) + half
    return np.round(lm, 3)


# name: (height, width, eye_left, eye_right, mouth centre, output_size, expected (shrink > 1, crop, pad))
CASES = {
    'inside': (100, 100, (39, 48), (61, 48), (50, 68), 48, (False, False, False)),
    'crop_only': (200, 220, (95, 90), (117, 92), (105, 111), 64, (False, True, False)),
    'pad_edge': (120, 110, (6, 50), (28, 53), (15, 72), 48, (False, True, True)),
    'pad_corner_rotated': (130, 150, (118, 22), (138, 30), (123, 45), 40, (False, True, True)),
    'shrink': (230, 250, (104, 105), (146.5, 105), (125, 144), 20, (True, True, False)),
    'shrink_pad': (180, 200, (150, 80), (192, 84), (170, 120), 20, (True, True, True)),
}


def main():
    ref_root = sys.argv[1]
    sys.modules.setdefault('dlib', types.ModuleType('dlib'))
    if not hasattr(PIL.Image, 'ANTIALIAS'):
        PIL.Image.ANTIALIAS = PIL.Image.LANCZOS
    spec = importlib.util.spec_from_file_location('ref_alignment', os.path.join(ref_root, 'utils', 'alignment.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    calls = []
    real_resize, real_crop, real_pad = PIL.Image.Image.resize, PIL.Image.Image.crop, np.pad
    PIL.Image.Image.resize = lambda self, *a, **k: (calls.append('resize'), real_resize(self, *a, **k))[1]
    PIL.Image.Image.crop = lambda self, *a, **k: (calls.append('crop'), real_crop(self, *a, **k))[1]
    np.pad = lambda *a, **k: (calls.append('pad'), real_pad(*a, **k))[1]

    out, seen = {}, set()
    with tempfile.TemporaryDirectory() as d:
        for i, (name, (h, w, el, er, mo, size, want)) in enumerate(CASES.items()):
            img = photo(h, w, 100 + i)
            assert img.nbytes < 200 * 1000, (name, img.nbytes)
            lm = landmarks(el, er, mo, 200 + i)
            path = os.path.join(d, name + '.png')
            PIL.Image.fromarray(img).save(path)                      # lossless: the reference reads back exactly `img`
            ref.get_landmark = lambda filepath, predictor, lm=lm: lm.copy()
            del calls[:]
            res = np.asarray(ref.align_face(path, None, size))
            got = ('resize' in calls, 'crop' in calls, 'pad' in calls)
            assert got == want, (name, got, want)
            assert res.shape == (size, size, 3) and res.dtype == np.uint8
            seen.add(got)
            out[name + '.image'] = img
            out[name + '.landmarks'] = lm
            out[name + '.output_size'] = np.int64(size)
            out[name + '.aligned'] = res
            out[name + '.branches'] = np.asarray(got)
            print(name, img.shape, '->', res.shape, dict(shrink=got[0], crop=got[1], pad=got[2]))
    PIL.Image.Image.resize, PIL.Image.Image.crop, np.pad = real_resize, real_crop, real_pad
    # every combination the tests need: nothing at all, crop only, pad without shrink, shrink without pad, shrink with pad
    for need in ((False, False, False), (False, True, False), (False, True, True), (True, True, False), (True, True, True)):
        assert need in seen, need
    assert len(CASES) >= 5
    path = os.path.join(HERE, 'align.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes')
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == '__main__':
    main()
