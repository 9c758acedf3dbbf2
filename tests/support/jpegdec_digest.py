"""Fresh-interpreter helper of tests/test_gpu_jpeg_decode.py: SHA-256 of the pixels and of the result words hipops.jpeg_decode gives for a few
cases of tests/support/jpegdec_cases.py at both subsequence sizes, printed as one JSON line -- run with EG3D_DETERMINISTIC=1 to use the
deterministic build, the way tests/support/jpeg_digest.py does.  csrc/jpeg_decode.hip holds no floating point and no data-carrying atomic: the
two builds must agree."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inv3d_amd import _lib as L, hipops as H  # noqa: E402
import jpegdec_cases as DC  # noqa: E402

NAMES = ('37x53_420', '40x72_422', 'grey_20x12', 'noise_q100_444', 'optimize_37x53_420', 'restart1_64x48_420', 'own_64x48_r3_444', DC.BIG)


def digests():
    out = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
    for name in NAMES:
        for B in DC.SUBSEQ:
            stats = {}
            px = H.jpeg_decode(DC.cases()[name], subseq_bytes=B, stats=stats)
            out[f'{name}@{B}'] = hashlib.sha256(px.cpu().numpy().tobytes() + json.dumps(stats, sort_keys=True).encode()).hexdigest()
    return out


if __name__ == '__main__':
    print(json.dumps(digests()))
