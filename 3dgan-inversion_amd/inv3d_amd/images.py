"""Target-image ingestion (utils/alignment.py, utils/align_data.py, utils/ImagesDataset.py, scripts/run_pti.py:28-30).

  align_plan, align_face   <- utils/alignment.py::align_face, lines 37-114: the geometry (quad, qsize, shrink, border, crop and pad boxes) in host
                              float64, statement by statement; every pixel step one of the kernels of csrc/imgprep.hip (hipops.pil_resize,
                              feather_pad, pil_quad_warp), the crop a slice.  Landmarks (68 x 2) come from a file, as in EG3D's preprocessing:
                              there is no landmark detector here
  paste_plan, paste_back   <- no reference counterpart (its alignment goes one way only): the inverse geometry of align_plan as one affine map
                              photo -> aligned frame in host float64, and the edited frame(s) blended back into the photograph by
                              hipops.paste_back (csrc/imgprep.hip): what tools/paste_back.py, video.write_orbit_video(paste=...),
                              tools/run_ganspace.py --paste-photo and tools/run_inversion.py --paste-back write; bands=1..6 | 'auto'
                              (paste_bands) blends through a Laplacian pyramid instead of the one alpha (hipops.paste_blend, csrc/blend.hip)
  e4e_image_transform      <- training/coaches/base_coach.py:41-45: ToPILImage, Resize((256, 256)), ToTensor, Normalize
  load_landmarks           <- a .json ({name: 68 x 2}) or .npz (one array per name) mapping
  load_targets             <- ImagesDataset / make_dataset + ToTensor / Normalize: the (name, target, None) tuples InversionCoach.run takes
  decode_rgb_batch,        no reference counterpart: many files per device decode (hipops.jpeg_decode_batch), and the frames of a Motion-JPEG
  video_targets               AVI (video.read_mjpeg_frames) as such tuples

PIL decodes the files on the host (imported lazily, and only in decode_rgb); decoder='gpu' moves the decode of baseline JPEG files to the
device as well (hipops.jpeg_decode, csrc/jpeg_decode.hip: the same bytes); everything after the decode runs on the device."""
import json
import math
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

IMG_EXTENSIONS = ('.jpg', '.JPG', '.jpeg', '.JPEG', '.png', '.PNG', '.ppm', '.PPM', '.bmp', '.BMP', '.tiff')      # utils/data_utils.py


class AlignPlan(NamedTuple):
    shrink_size: Optional[Tuple[int, int]]         # (width, height) of the LANCZOS shrink, or None
    crop: Optional[Tuple[int, int, int, int]]      # (x0, y0, x1, y1) in the (shrunk) image, or None
    pad: Optional[Tuple[int, int, int, int]]       # (left, top, right, bottom), or None
    qsize: float                                   # at the pad step (after the shrink)
    quad: Tuple[float, ...]                        # the QUAD transform's data: NW, SW, SE, NE corners + 0.5, in the padded image


def align_plan(height: int, width: int, landmarks, output_size: int) -> AlignPlan:
    """The host geometry of align_face for an image of height x width (alignment.py:37-109, statement by statement, float64)."""
    lm = np.asarray(landmarks)
    if lm.shape != (68, 2):
        raise ValueError(f'align_plan: landmarks 68 x 2, got {lm.shape}')
    lm_eye_left = lm[36: 42]  # left-clockwise
    lm_eye_right = lm[42: 48]  # left-clockwise
    lm_mouth_outer = lm[48: 60]  # left-clockwise

    # Calculate auxiliary vectors.
    eye_left = np.mean(lm_eye_left, axis=0)
    eye_right = np.mean(lm_eye_right, axis=0)
    eye_avg = (eye_left + eye_right) * 0.5
    eye_to_eye = eye_right - eye_left
    mouth_left = lm_mouth_outer[0]
    mouth_right = lm_mouth_outer[6]
    mouth_avg = (mouth_left + mouth_right) * 0.5
    eye_to_mouth = mouth_avg - eye_avg

    # Choose oriented crop rectangle.
    x = eye_to_eye - np.flipud(eye_to_mouth) * [-1, 1]
    x /= np.hypot(*x)
    x *= max(np.hypot(*eye_to_eye) * 2.0, np.hypot(*eye_to_mouth) * 1.8)
    y = np.flipud(x) * [-1, 1]
    c = eye_avg + eye_to_mouth * 0.1
    quad = np.stack([c - x - y, c - x + y, c + x + y, c + x - y])
    qsize = np.hypot(*x) * 2

    size = [int(width), int(height)]                 # img.size

    # Shrink.
    shrink_size = None
    shrink = int(np.floor(qsize / output_size * 0.5))
    if shrink > 1:
        shrink_size = (int(np.rint(float(size[0]) / shrink)), int(np.rint(float(size[1]) / shrink)))
        size = list(shrink_size)
        quad /= shrink
        qsize /= shrink

    # Crop.
    crop_box = None
    border = max(int(np.rint(qsize * 0.1)), 3)
    crop = (int(np.floor(min(quad[:, 0]))), int(np.floor(min(quad[:, 1]))), int(np.ceil(max(quad[:, 0]))), int(np.ceil(max(quad[:, 1]))))
    crop = (max(crop[0] - border, 0), max(crop[1] - border, 0), min(crop[2] + border, size[0]), min(crop[3] + border, size[1]))
    if crop[2] - crop[0] < size[0] or crop[3] - crop[1] < size[1]:
        crop_box = crop
        size = [crop[2] - crop[0], crop[3] - crop[1]]
        quad -= crop[0:2]

    # Pad.
    pad_box = None
    pad = (int(np.floor(min(quad[:, 0]))), int(np.floor(min(quad[:, 1]))), int(np.ceil(max(quad[:, 0]))), int(np.ceil(max(quad[:, 1]))))
    pad = (max(-pad[0] + border, 0), max(-pad[1] + border, 0), max(pad[2] - size[0] + border, 0), max(pad[3] - size[1] + border, 0))
    if max(pad) > border - 4:                        # enable_padding is True in the reference
        pad = np.maximum(pad, int(np.rint(qsize * 0.3)))
        pad_box = tuple(int(v) for v in pad)
        quad += pad[:2]

    return AlignPlan(shrink_size, crop_box, pad_box, float(qsize), tuple(float(v) for v in (quad + 0.5).flatten()))


def align_face(img_u8: torch.Tensor, landmarks, output_size: int) -> torch.Tensor:
    """utils/alignment.py::align_face on the device: uint8 [H,W,3] (the decoded photograph) and its 68 x 2 landmarks -> the aligned uint8
    [output_size, output_size, 3] image.  Byte-equal to the reference's Pillow calls unless the pad branch runs (fp32 there)."""
    from . import hipops
    if img_u8.dim() != 3:
        raise ValueError(f'align_face: one uint8 [H,W,C] image, got {tuple(img_u8.shape)}')
    plan = align_plan(img_u8.shape[0], img_u8.shape[1], landmarks, output_size)
    img = img_u8
    if plan.shrink_size is not None:
        img = hipops.pil_resize(img, plan.shrink_size, 'lanczos')                 # PIL.Image.ANTIALIAS is LANCZOS
    if plan.crop is not None:
        x0, y0, x1, y1 = plan.crop
        img = img[y0:y1, x0:x1]
    if plan.pad is not None:
        img = hipops.feather_pad(img, plan.pad, plan.qsize)
    # transform_size = output_size in the reference, so its closing `if output_size < transform_size: img.resize(...)` (alignment.py:110-111)
    # is dead code: the warp writes the output size directly, and it stays dead here
    return hipops.pil_quad_warp(img, (output_size, output_size), plan.quad)


class PastePlan(NamedTuple):
    matrix: Tuple[float, ...]                      # m0..m5: u = m0 + m1 X + m2 Y, v = m3 + m4 X + m5 Y, photo -> aligned frame (centres at + 0.5)
    region: Tuple[int, int, int, int]              # (x0, y0, x1, y1): the aligned square's bounding box in the photo, clamped to it
    presize: Optional[int]                         # side to shrink the edit to before the paste (scale > 1), or None
    scale: float                                   # aligned pixels per photo pixel


def paste_plan(height: int, width: int, landmarks, output_size: int) -> PastePlan:
    """The inverse geometry of align_face for a photograph of height x width and an aligned frame of output_size (host float64).  align_face
    is shrink, crop, pad, QUAD warp; the quad is a rotated square, so the QUAD map is affine and photo -> aligned frame is one affine map:
        P = (X sx + ox, Y sy + oy),  (u, v) = A^-1 (P - (a0, a4))
    with sx, sy = the scale the LANCZOS shrink really applied (shrunk size / size, not 1 / shrink), (ox, oy) = pad - crop offsets and
    a0..a7 = hipops.pil_quad_coeffs of the plan's quad.  A general quad (bilinear coefficients a3, a7 that matter) has no such inverse and
    raises ValueError.  No reference counterpart: the reference's alignment goes one way only."""
    from .hipops import pil_quad_coeffs
    S = int(output_size)
    plan = align_plan(height, width, landmarks, S)
    a = pil_quad_coeffs((S, S), plan.quad)
    if not np.isfinite(a).all() or max(abs(a[3]), abs(a[7])) * S * S > 1e-6:
        raise ValueError('paste_plan: the quad is no parallelogram: a general quad is not a supported inverse')
    det = a[1] * a[6] - a[2] * a[5]
    if det == 0.0:
        raise ValueError('paste_plan: a degenerate quad')
    sx = plan.shrink_size[0] / float(width) if plan.shrink_size is not None else 1.0
    sy = plan.shrink_size[1] / float(height) if plan.shrink_size is not None else 1.0
    ox = float((plan.pad[0] if plan.pad is not None else 0) - (plan.crop[0] if plan.crop is not None else 0))
    oy = float((plan.pad[1] if plan.pad is not None else 0) - (plan.crop[1] if plan.crop is not None else 0))
    i00, i01, i10, i11 = a[6] / det, -a[2] / det, -a[5] / det, a[1] / det          # A^-1
    tx, ty = ox - a[0], oy - a[4]
    matrix = (i00 * tx + i01 * ty, i00 * sx, i01 * sy, i10 * tx + i11 * ty, i10 * sx, i11 * sy)
    # the square's corners pulled back to the photo: X = (a0 + a1 u + a2 v - ox) / sx
    xs = [(a[0] + a[1] * u + a[2] * v - ox) / sx for u, v in ((0, 0), (0, S), (S, S), (S, 0))]
    ys = [(a[4] + a[5] * u + a[6] * v - oy) / sy for u, v in ((0, 0), (0, S), (S, S), (S, 0))]
    clamp = lambda v, hi: int(min(max(v, 0), hi))
    region = (clamp(np.floor(min(xs)), width), clamp(np.floor(min(ys)), height), clamp(np.ceil(max(xs)), width), clamp(np.ceil(max(ys)), height))
    scale = float(np.sqrt(abs(matrix[1] * matrix[5] - matrix[2] * matrix[4])))
    presize = max(1, int(np.rint(S / scale))) if scale > 1.0 else None
    return PastePlan(tuple(float(v) for v in matrix), region, presize, scale)


def _edit_frames(edit: torch.Tensor):
    """uint8 [N,S,S,3] frames (and whether the frame axis was added) of what paste_back accepts."""
    from . import hipops
    if edit.dtype == torch.uint8 and edit.dim() in (3, 4) and edit.shape[-1] == 3 and edit.shape[-2] == edit.shape[-3]:
        return (edit[None] if edit.dim() == 3 else edit), edit.dim() == 3
    if edit.dtype == torch.float32 and edit.dim() == 4 and edit.shape[1] == 3 and edit.shape[2] == edit.shape[3]:
        n, _, s, _ = edit.shape
        return hipops.image_grid_u8(edit, nrow=1, padding=0).reshape(n, s, s, 3), False
    raise ValueError(f'paste_back: edit uint8 [S,S,3] or [N,S,S,3], or fp32 [N,3,S,S] in [-1,1], got {tuple(edit.shape)} {edit.dtype}')


def paste_bands(plan: PastePlan, S: int, feather: float) -> int:
    """The bands paste_back(bands='auto') uses: clamp(floor(log2(max(2, feather S / scale))) - 1, 1, 5) -- the broadest band's transition
    (about 2^(bands + 1) photo pixels) is about the feather's width in photo pixels.  A geometric choice, not tuned on real heads."""
    width = max(2.0, float(feather) * float(S) / float(plan.scale))
    return int(min(max(int(np.floor(np.log2(width))) - 1, 1), 5))


def bands_arg(text: str):
    """The text of the tools' --paste-bands as paste_back's bands: 0 (the one-alpha blend), 1..6, or 'auto' (paste_bands); else ValueError."""
    if text == 'auto':
        return text
    n = int(text)
    if not 0 <= n <= 6:
        raise ValueError(f"bands 0..6 or 'auto', got {text!r}")
    return n


def paste_back(photo_u8: torch.Tensor, edit: torch.Tensor, landmarks, feather: float = 0.08, mask: Optional[torch.Tensor] = None,
               region: str = 'photo', layout: str = 'hwc', bands=0) -> torch.Tensor:
    """The closing step of an edit: the aligned S x S result(s) blended back into the photograph they were aligned from, on the device
    (hipops.paste_back).  photo_u8 uint8 [H,W,3] and the landmarks align_face took; edit uint8 [S,S,3] or [N,S,S,3], or the generator's fp32
    [N,3,S,S] in [-1,1] (quantised as hipops.image_grid_u8 does) -- S is the edit's own side, whatever side the photo was aligned at.
    feather = the blend ramp from the frame's edge as a fraction of the side; mask = uint8 [S,S] or [N,S,S] in the aligned frame.
    region='photo': the whole photograph per frame ([H,W,3] for one [S,S,3] edit, else [N,H,W,3]); a face wholly outside the photo gives the
    photo unchanged.  region='bbox': only the aligned square's bounding box in the photo (PastePlan.region); ValueError if that is empty.
    Where the face is smaller in the photo than in the frame (PastePlan.scale > 1) the edit and the mask are first shrunk to presize with
    Pillow's LANCZOS (hipops.pil_resize), so the bilinear taps do not alias.  layout='chw' gives [N,3,H,W] for the JPEG encoder.
    bands=0: the one-alpha blend (hipops.paste_back).  bands=1..6: the multi-band blend (hipops.paste_blend) after the same presize -- the
    coarse part of edit - photo fades over a wide transition, the detail over a narrow one, which hides the tone seam a render leaves around
    the head; the result has the same shape (region='bbox' drops what the blend changes outside the box).  bands='auto': paste_bands."""
    from . import hipops
    if region not in ('photo', 'bbox'):
        raise ValueError(f"paste_back: region 'photo' | 'bbox', got {region!r}")
    if not (bands == 'auto' or (isinstance(bands, (int, np.integer)) and not isinstance(bands, bool) and 0 <= int(bands) <= 6)):
        raise ValueError(f"paste_back: bands 0..6 or 'auto', got {bands!r}")
    if photo_u8.dim() != 3:
        raise ValueError(f'paste_back: one uint8 [H,W,3] photo, got {tuple(photo_u8.shape)}')
    frames, squeeze = _edit_frames(edit)
    S = int(frames.shape[1])
    plan = paste_plan(photo_u8.shape[0], photo_u8.shape[1], landmarks, S)
    x0, y0, x1, y1 = plan.region
    if region == 'bbox' and (x1 <= x0 or y1 <= y0):
        raise ValueError('paste_back: the aligned square lies wholly outside the photo')
    matrix, feather_px = np.asarray(plan.matrix, dtype=np.float64), float(feather) * S
    if mask is not None and mask.dim() not in (2, 3):
        raise ValueError(f'paste_back: mask uint8 [S,S] or [N,S,S], got {tuple(mask.shape)}')
    if plan.presize is not None and plan.presize != S:
        ps = plan.presize
        frames = hipops.pil_resize(frames, (ps, ps), 'lanczos')
        if mask is not None:
            mask = hipops.pil_resize(mask[..., None], (ps, ps), 'lanczos')[..., 0]
        matrix, feather_px = matrix * (ps / S), feather_px * (ps / S)
    bands = paste_bands(plan, S, feather) if bands == 'auto' else int(bands)
    if bands == 0:
        out = hipops.paste_back(photo_u8, frames, matrix, plan.region, feather_px=feather_px, mask=mask, whole=region == 'photo', layout=layout)
    else:
        out = hipops.paste_blend(photo_u8, frames, matrix, plan.region, bands, feather_px=feather_px, mask=mask, whole=region == 'photo',
                                 layout=layout)
    return out[0] if squeeze else out


def foreground_mask(depth: torch.Tensor) -> torch.Tensor:
    """The reference's foreground (training/warping_loss.py:12-16: depth < mean(depth)) per frame: image_depth fp32 [N,1,h,w] -> uint8 [N,h,w],
    255 where the pixel is nearer than its own frame's mean depth (the reference's batch is 1, so its mean is a frame's)."""
    if depth.dim() != 4 or depth.shape[1] != 1 or not depth.is_floating_point():
        raise ValueError(f'foreground_mask: image_depth [N,1,h,w], got {tuple(depth.shape)} {depth.dtype}')
    d = depth.float()
    return (d < d.mean(dim=(1, 2, 3), keepdim=True))[:, 0].to(torch.uint8) * 255


def matte_thresholds(side: int, open: float = 0.02, close: float = 0.04) -> Tuple[int, ...]:
    """hipops.edt2's stage thresholds for a mask of `side` rows: open (erode, dilate) then close (dilate, erode), the radii fractions of the
    side; a zero radius drops its two stages.  r = frac * side in float64; erode by r is floor(r^2), dilate by r is -floor(r^2) - 1."""
    t = []
    for name, frac, erode_first in (('open', open, True), ('close', close, False)):
        r = float(frac) * int(side)
        if not r >= 0.0:
            raise ValueError(f'matte_from_mask: {name} >= 0, got {frac}')
        if r > 0.0:
            q = int(math.floor(r * r))
            t += [q, -q - 1] if erode_first else [-q - 1, q]
    return tuple(t)


def matte_from_mask(mask_u8: torch.Tensor, size: int, open: float = 0.02, close: float = 0.04, shrink: float = 0.0, feather: float = 0.03,
                    impl: str = 'auto') -> torch.Tensor:
    """A ragged binary mask uint8 [N,s,s] (or [s,s]; foreground = nonzero) in the aligned frame -> the soft matte uint8 [N,size,size] paste_back
    takes as `mask`, on the device without a host synchronise (hipops.edt2, hipops.matte8; no reference counterpart).  open removes specks
    (erode, dilate), close fills holes (dilate, erode): disc radii as fractions of the mask's side, 0 drops the pair.  The edge is then placed
    at sub-pixel precision at `size`, moved inwards by shrink and ramped over feather (smoothstep), both fractions of `size` -- as paste_back's
    feather is a fraction of its side."""
    from . import hipops
    if mask_u8.dim() not in (2, 3) or mask_u8.shape[-1] != mask_u8.shape[-2]:
        raise ValueError(f'matte_from_mask: a square uint8 mask [N,s,s] or [s,s], got {tuple(mask_u8.shape)}')
    size = int(size)
    sd2 = hipops.edt2(mask_u8, matte_thresholds(mask_u8.shape[-2], open, close), impl=impl)
    return hipops.matte8(sd2, size, shrink_px=float(shrink) * size, feather_px=float(feather) * size)


@torch.no_grad()
def head_matte(G, ws: torch.Tensor, cam: torch.Tensor, size: Optional[int] = None, source: str = 'depth', depth: Optional[torch.Tensor] = None,
               shape_kwargs: Optional[dict] = None, **matte_kwargs) -> torch.Tensor:
    """The head's soft matte uint8 [N,size,size] for the frames G.synthesis(ws, cam) renders (size defaults to G.img_resolution), what
    paste_back(mask=...) takes so that the photograph's own background stays around the head.  No reference counterpart.
    source='depth' (the default): foreground_mask of image_depth at the neural-rendering resolution -- of `depth` [N,1,h,w] where the caller
    already has the frame's render (no second one), else of G.synthesis(ws, cam, noise_mode='const').
    source='shape': inference.render_shape(G, ws, cam, res=size, **shape_kwargs)['mask'], the first-hit mask of the density surface at full
    resolution (one latent, N cameras).  EG3D's FFHQ density contains the wall behind the head, which this mask then contains too: it is for
    grids cleaned with shape_kwargs=dict(keep=...), and 'depth' is the default for that reason.
    matte_kwargs go to matte_from_mask (open, close, shrink, feather, impl)."""
    size = int(G.img_resolution if size is None else size)
    if source == 'depth':
        if depth is None:
            depth = G.synthesis(ws, cam, noise_mode='const')['image_depth']
        mask = foreground_mask(depth)
    elif source == 'shape':
        from .inference import render_shape
        m = render_shape(G, ws, cam, res=size, **(shape_kwargs or {}))['mask']
        mask = (m.reshape(-1, size, size) != 0).to(torch.uint8) * 255
    else:
        raise ValueError(f"head_matte: source 'depth' | 'shape', got {source!r}")
    return matte_from_mask(mask, size, **matte_kwargs)


def e4e_image_transform(target: torch.Tensor) -> torch.Tensor:
    """base_coach.py:41-45 applied to (target + 1) / 2 as the coach applies it: fp32 [N,3,H,W] in [0,1] -> ToPILImage (mul(255).byte()),
    PIL Resize((256, 256)) (bilinear, on uint8), ToTensor, Normalize(0.5, 0.5) -> fp32 [N,3,256,256].  Offered as a function: the coach's own
    start-latent path is unchanged."""
    from . import hipops
    if target.dim() != 4 or target.shape[1] != 3 or not target.dtype.is_floating_point:
        raise ValueError(f'e4e_image_transform: floating-point [N,3,H,W] in [0,1], got {tuple(target.shape)} {target.dtype}')
    u8 = target.mul(255).byte().permute(0, 2, 3, 1).contiguous()
    return hipops.u8_to_target(hipops.pil_resize(u8, (256, 256), 'bilinear'))


def load_landmarks(path: str) -> dict:
    """{name: float64 [68,2]} from a .json ({name: [[x, y], ...]}) or an .npz (one array per name).  Names are file names up to their first dot."""
    if path.endswith('.npz'):
        with np.load(path, allow_pickle=False) as z:
            out = {k: np.asarray(z[k], dtype=np.float64) for k in z.files}
    else:
        with open(path) as f:
            out = {k: np.asarray(v, dtype=np.float64) for k, v in json.load(f).items()}
    for k, v in out.items():
        if v.shape != (68, 2):
            raise ValueError(f'load_landmarks: {k}: 68 x 2 expected, got {v.shape}')
    return out


def image_files(directory: str):
    """[(name, path)] of the image files under a directory, sorted: ImagesDataset's `sorted(make_dataset(root))` -- the tree is walked, the
    name is the file name up to its first dot (utils/data_utils.py:25-34)."""
    if not os.path.isdir(directory):
        raise ValueError(f'{directory} is not a valid directory')
    out = []
    for root, _, fnames in sorted(os.walk(directory)):
        for fname in fnames:
            if fname.endswith(IMG_EXTENSIONS):
                out.append((fname.split('.')[0], os.path.join(root, fname)))
    return sorted(out)


DECODERS = ('pil', 'gpu')
JPEG_EXTENSIONS = ('.jpg', '.jpeg')


def decode_rgb(path: str, device, decoder: str = 'pil', report=None) -> torch.Tensor:
    """uint8 [H,W,3] on the device: PIL.Image.open(path).convert('RGB').  decoder='pil': the decode is host work.  decoder='gpu': a file
    whose name ends in .jpg / .jpeg (any case) is decoded on the device by hipops.jpeg_decode, to the same bytes; a JPEG the device decoder
    does not take (video.JpegUnsupported: progressive, CMYK, ...) or refuses (a damaged stream: hipops.JpegDecodeRefused) and every other format take the
    PIL path, so a bad file behaves as it does with decoder='pil'.  report(path, reason), if given, is told about every such JPEG."""
    if decoder not in DECODERS:
        raise ValueError(f'decode_rgb: decoder one of {DECODERS}, got {decoder!r}')
    if decoder == 'gpu' and path.lower().endswith(JPEG_EXTENSIONS):
        from . import hipops
        from .video import JpegUnsupported
        try:
            with open(path, 'rb') as f:
                data = f.read()
            return hipops.jpeg_decode(data, device=device)
        except (JpegUnsupported, hipops.JpegDecodeRefused) as e:                   # (any other error -- a failed launch, no GPU -- is the caller's)
            if report is not None:
                report(path, str(e))
    from PIL import Image
    with Image.open(path) as im:
        arr = np.array(im.convert('RGB'), dtype=np.uint8)
    return torch.from_numpy(arr).to(device)


def decode_rgb_batch(paths, device, decoder: str = 'pil', report=None) -> list:
    """[uint8 [H,W,3] on the device per path]: decode_rgb of every path, the same bytes and the same fallback rule per file.  decoder='gpu':
    the files named .jpg / .jpeg go through ONE hipops.jpeg_decode_batch (one upload, the launches of a single decode, one synchronise for
    all of them, whatever their sizes); those the device decoder does not take or refuses, and every other format, take the PIL path, and
    report(path, reason) is told about every such JPEG, once."""
    if decoder not in DECODERS:
        raise ValueError(f'decode_rgb_batch: decoder one of {DECODERS}, got {decoder!r}')
    paths = list(paths)
    out = [None] * len(paths)
    jpegs = [i for i, p in enumerate(paths) if p.lower().endswith(JPEG_EXTENSIONS)] if decoder == 'gpu' else []
    if jpegs:
        from . import hipops
        files = []
        for i in jpegs:
            with open(paths[i], 'rb') as f:
                files.append(f.read())
        for i, got in zip(jpegs, hipops.jpeg_decode_batch(files, device=device, return_errors=True)):
            if isinstance(got, Exception):
                if report is not None:
                    report(paths[i], str(got))
            else:
                out[i] = got
    return [decode_rgb(p, device, 'pil') if o is None else o for p, o in zip(paths, out)]


def _decoded(files, device, decoder: str, report, decode_batch: int):
    """(name, path, uint8 [H,W,3]) over [(name, path)]: decode_rgb per file (decode_batch = 1), or decode_rgb_batch of decode_batch files."""
    if decode_batch < 1:
        raise ValueError(f'decode_batch >= 1, got {decode_batch}')
    if decode_batch == 1:
        for name, path in files:
            yield name, path, decode_rgb(path, device, decoder, report)
        return
    for k in range(0, len(files), decode_batch):
        block = files[k:k + decode_batch]
        for (name, path), img in zip(block, decode_rgb_batch([p for _, p in block], device, decoder, report)):
            yield name, path, img


def write_aligned(directory: str, landmarks, out_dir: str, output_size: int = 512, device='cuda', png_encoder: str = 'host', batch: int = 8,
                  report=None, decoder: str = 'pil', decode_report=None, decode_batch: int = 1):
    """{out_dir}/{name}.png for every image file of `directory` whose name has landmarks ({name: 68 x 2}, or the path of a .json / .npz):
    decoded on the host, aligned by align_face, written by video.write_png.  png_encoder='gpu': the aligned frames -- all output_size squared
    -- go `batch` at a time through one video.write_pngs (one encode, one copy).  Files without landmarks are passed to `report(path)` and
    skipped.  decoder='gpu': JPEG files are decoded on the device too (decode_rgb; decode_report(path, reason) hears of every JPEG that took
    the PIL path instead); the files written are the same.  decode_batch > 1: the files with landmarks are decoded that many at a time
    (decode_rgb_batch), to the same files in the same order.  Returns the paths written."""
    from . import video
    if decoder not in DECODERS:
        raise ValueError(f'write_aligned: decoder one of {DECODERS}, got {decoder!r}')
    if png_encoder not in video.PNG_ENCODERS or batch < 1:
        raise ValueError(f'write_aligned: png_encoder one of {video.PNG_ENCODERS} and batch >= 1, got {png_encoder!r}, {batch}')
    if isinstance(landmarks, str):
        landmarks = load_landmarks(landmarks)
    os.makedirs(out_dir, exist_ok=True)
    written, pending = [], []

    def flush():
        if pending:
            video.write_pngs([p for p, _ in pending], torch.stack([f for _, f in pending]))
            pending.clear()
    files = []
    for name, path in image_files(directory):
        if name in landmarks:
            files.append((name, path))
        elif report is not None:
            report(path)
    for name, path, img in _decoded(files, device, decoder, decode_report, decode_batch):
        out = os.path.join(out_dir, name + '.png')
        frame = align_face(img, landmarks[name], output_size)
        if png_encoder == 'gpu':
            pending.append((out, frame))
            if len(pending) == batch:
                flush()
        else:
            video.write_png(out, frame)
        written.append(out)
    flush()
    return written


def load_targets(directory: str, landmarks=None, output_size: int = 512, device='cuda', decoder: str = 'pil', decode_report=None,
                 decode_batch: int = 1):
    """[(name, target fp32 [1,3,S,S] in [-1,1] on the device, None)] for InversionCoach.run, S = output_size: every image file of `directory` in
    sorted order, decoded to RGB; aligned by align_face where `landmarks` (a {name: 68 x 2} mapping, or the path of a .json / .npz holding
    one) has its name, otherwise required to be S x S already; then ToTensor + Normalize(0.5, 0.5) (hipops.u8_to_target).  decoder='gpu':
    JPEG files are decoded on the device (decode_rgb), to the same targets.  decode_batch > 1: the files are decoded that many at a time
    (decode_rgb_batch), to the same targets in the same order."""
    from . import hipops
    if decoder not in DECODERS:
        raise ValueError(f'load_targets: decoder one of {DECODERS}, got {decoder!r}')
    if isinstance(landmarks, str):
        landmarks = load_landmarks(landmarks)
    landmarks = landmarks or {}
    out = []
    for name, path, img in _decoded(image_files(directory), device, decoder, decode_report, decode_batch):
        if name in landmarks:
            img = align_face(img, landmarks[name], output_size)
        elif tuple(img.shape[:2]) != (output_size, output_size):
            raise ValueError(f'load_targets: {path} is {img.shape[1]} x {img.shape[0]} and has no landmarks: give landmarks for it or a '
                             f'{output_size} x {output_size} image')
        out.append((name, hipops.u8_to_target(img), None))
    return out


def video_targets(path: str, landmarks=None, frames: slice = slice(None), output_size: int = 512, device='cuda', batch: int = 16, decoder: str = 'gpu',
                  decode_report=None):
    """load_targets for the frames of a Motion-JPEG AVI (video.read_mjpeg_frames: `batch` frames per device decode): [(name, target fp32
    [1,3,S,S] in [-1,1] on the device, None)] for frames[start:stop:step] of the file, name = f'{stem}_{index:06d}' with the file's name up
    to its first dot and the frame's index in the file.  A frame is aligned by align_face where `landmarks` ({name: 68 x 2}, or the path of
    a .json / .npz) has its name; otherwise it is required to be S x S already."""
    from . import hipops, video
    if isinstance(landmarks, str):
        landmarks = load_landmarks(landmarks)
    landmarks = landmarks or {}
    stem = os.path.basename(path).split('.')[0]
    step = 1 if frames.step is None else frames.step
    out = []
    for first, block in video.read_mjpeg_frames(path, frames.start, frames.stop, step, batch=batch, device=device, decoder=decoder, report=decode_report):
        for j in range(block.shape[0]):
            name, img = f'{stem}_{first + j * step:06d}', block[j]
            if name in landmarks:
                img = align_face(img, landmarks[name], output_size)
            elif tuple(img.shape[:2]) != (output_size, output_size):
                raise ValueError(f'video_targets: frame {first + j * step} of {path} is {img.shape[1]} x {img.shape[0]} and has no landmarks: give '
                                 f'landmarks for {name} or a {output_size} x {output_size} video')
            out.append((name, hipops.u8_to_target(img), None))
    return out
