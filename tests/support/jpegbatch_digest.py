"""Fresh-interpreter helper of tests/test_gpu_jpeg_batch.py: SHA-256 of the pixels and of the per-image stats hipops.jpeg_decode_batch gives for
ALL cases of tests/support/jpegdec_cases.py in one call, at both subsequence sizes, printed as one JSON line -- run with EG3D_DETERMINISTIC=1
to use the deterministic build, the way tests/support/jpegdec_digest.py does for the one-image call."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, '3dgan-inversion_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inv3d_amd import _lib as L, hipops as H  # noqa: E402
import jpegdec_cases as DC  # noqa: E402


def digests():
    out = dict(deterministic_build=bool(L.lib().eg3d_det_enabled()))
    names = list(DC.cases())
    for B in DC.SUBSEQ:
        stats = []
        px = H.jpeg_decode_batch([DC.cases()[n] for n in names], subseq_bytes=B, stats=stats)
        for name, p, s in zip(names, px, stats):
            out[f'{name}@{B}'] = hashlib.sha256(p.cpu().numpy().tobytes() + json.dumps(s, sort_keys=True).encode()).hexdigest()
    return out


if __name__ == '__main__':
    print(json.dumps(digests()))
