"""Helpers shared by tests/test_jpeg_batch_cpu.py and tests/test_gpu_jpeg_batch.py: JPEG files with their DHT segments removed (what
Motion-JPEG writers emit), Motion-JPEG AVI files and their variants, the damage recipes of test_damaged_stream_ends_in_a_status, and the many
distinct tiny files of the N = 1025 batch.  Nothing here touches the GPU."""
import functools
import io
import struct

import numpy as np

import jpeg_cases as JC
import jpegdec_cases as DC


def strip_dht(data: bytes) -> bytes:
    """The file without its DHT (FF C4) segments; everything from SOS on is copied as it stands."""
    out, pos = bytearray(data[:2]), 2
    while True:
        assert data[pos] == 0xFF, pos
        marker = data[pos + 1]
        length = struct.unpack_from('>H', data, pos + 2)[0]
        if marker == 0xDA:
            return bytes(out) + data[pos:]
        if marker != 0xC4:
            out += data[pos:pos + 2 + length]
        pos += 2 + length


def pil_rgb(data: bytes) -> np.ndarray:
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert('RGB'), dtype=np.uint8)


def write_avi(path: str, frames, width: int, height: int, fps: int = 30) -> None:
    from inv3d_amd import video as V
    with V.MjpegAviWriter(path, width, height, fps=fps) as w:
        for f in frames:
            w.write(f)


def avi_without_index(data: bytes) -> bytes:
    """The file cut before 'idx1', the RIFF size patched."""
    at = data.rindex(b'idx1')
    return data[:4] + struct.pack('<I', at - 8) + data[8:at]


def avi_with_file_offsets(data: bytes) -> bytes:
    """The 'idx1' offsets rewritten from 'movi'-relative to file-relative (the other convention in the wild)."""
    at, movi = data.rindex(b'idx1'), data.index(b'movi')
    n = struct.unpack_from('<I', data, at + 4)[0] // 16
    out = bytearray(data)
    for i in range(n):
        e = at + 8 + 16 * i + 8
        out[e:e + 4] = struct.pack('<I', struct.unpack_from('<I', data, e)[0] + movi)
    return bytes(out)


def truncated(data: bytes) -> bytes:
    """Half the entropy-coded segment with EOI re-appended."""
    from inv3d_amd import video as V
    p = V.jpeg_scan_plan(data)
    return data[:p.scan_start + (p.scan_end - p.scan_start) // 2] + b'\xff\xd9'


def stray_marker(data: bytes) -> bytes:
    """A restart marker the geometry does not have, 40 bytes into the entropy-coded segment."""
    from inv3d_amd import video as V
    p = V.jpeg_scan_plan(data)
    out = bytearray(data)
    out[p.scan_start + 40:p.scan_start + 42] = b'\xff\xd3'
    return bytes(out)


def progressive_file() -> bytes:
    return DC.pil_file(JC.textured(40, 56, 90), 85, 2, progressive=True)


@functools.lru_cache(maxsize=None)
def tiny_files(n: int = 1025):
    """n files of 8 x 8 (4:4:4) and 1 x 1 (4:2:0) random pixels, a few hundred bytes each, and PIL's decode of each (read-only)."""
    rng = np.random.RandomState(1025)
    files = []
    for i in range(n):
        if i % 2 == 0:
            files.append(DC.pil_file(rng.randint(0, 256, (3, 8, 8)).astype(np.uint8), 90, 0))
        else:
            files.append(DC.pil_file(rng.randint(0, 256, (3, 1, 1)).astype(np.uint8), 100, 2))
    return tuple(files), tuple(pil_rgb(f) for f in files)
