"""GANSpace latent editing (the reference's ganspace/ directory) on the gfx950 kernels of csrc/pca.hip.

  FRONT_CAM, sample_w, fit_w_pca    <- ganspace/pca_anlaysis.py: 10^5 latents through G.mapping at a fixed frontal camera, a PCA of the first row of W
  fit_pca, PCAResult                <- ganspace/estimator.py PCAEstimator.fit / get_components (sklearn PCA, svd_solver='full'): here second moments
                                       accumulated chunk by chunk on the device (hipops.pca_moments), the covariance's eigenvectors from the Jacobi solver
                                       (hipops.sym_eig); no sklearn, nothing of W on the host
  save_components, load_components  <- the [K, D] float32 .npy files of ganspace/pca_comp/
  edit_directions, edit_ganspace    <- ganspace/run_ganspace.py:21-57 (the row of edits and its make_grid image; bytes from hipops.image_grid_u8,
                                       no torchvision)
  edit_orbit                        <- inference.render_orbit of every edited latent
  GANSPACE_DIRECTIONS               <- the sample table of run_ganspace.py:71-78

Differences from the reference: the fit streams W in chunks (the reference holds 10^5 x 14 x 512 floats on the device and a copy on the host); a
layer range that does not fit and fewer than two images raise ValueError (the reference prints and returns None / divides by zero)."""
from typing import Iterable, Iterator, NamedTuple, Optional

import numpy as np
import torch

from . import hipops as H
from ._lib import Eg3dHipError

# the conditioning camera of pca_anlaysis.py:13-25 (cam2world 4x4, intrinsics 3x3)
FRONT_CAM = (0.9966070652008057, 0.003541737562045455, -0.08222994953393936, 0.20670529656089412,
             -0.009605886414647102, -0.9872410893440247, -0.15894262492656708, 0.4137044218920643,
             -0.08174371719360352, 0.1591932326555252, -0.9838574528694153, 2.660098037982929,
             0, 0, 0, 1,
             4.2647, 0, 0.5, 0, 4.2647, 0.5, 0, 0, 1)

# name -> (idx_comp, start_layer, layer_num, edit_power), run_ganspace.py:71-78 ("ONLY sample parameters")
GANSPACE_DIRECTIONS = {
    'bright hair': (2, 7, 7, 4),
    'smile': (12, 0, 5, 2),
    'age': (5, 0, 5, 3.5),
    'short hair': (2, 0, 5, 4),
    'glass': (4, 0, 5, 4),
    'gender': (0, 0, 5, 4),
}


class PCAResult(NamedTuple):
    components: torch.Tensor      # [K, D] rows, by descending projected standard deviation; largest-magnitude entry of a row positive
    stdev: torch.Tensor           # [K] standard deviation (ddof 0) of the centred data along each component
    var_ratio: torch.Tensor       # [K] stdev^2 / total_var
    mean: torch.Tensor            # [D]
    total_var: float              # trace of the ddof-0 covariance
    n_samples: int
    sweeps: int
    converged: bool


@torch.no_grad()
def sample_w(G, n_samples: int, seed: int = 0, cam=FRONT_CAM, chunk: int = 8192) -> Iterator[torch.Tensor]:
    """Yields [<= chunk, w_dim] chunks of G.mapping(z, cam)[:, 0, :] (truncation_psi 1) for n_samples z ~ N(0, 1) from a device generator
    seeded with `seed`: the same (seed, chunk) gives the same rows."""
    dev = next(G.parameters()).device
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    c = torch.as_tensor(cam, dtype=torch.float32, device=dev).reshape(1, 25)
    for head in range(0, int(n_samples), int(chunk)):
        n = min(int(chunk), int(n_samples) - head)
        z = torch.randn((n, G.z_dim), generator=gen, device=dev)
        yield G.mapping(z, c.expand(n, -1))[:, 0, :].float()


def fit_pca(chunks: Iterable[torch.Tensor], n_components: Optional[int] = None, max_sweeps: int = 60) -> PCAResult:
    """PCA of the rows of `chunks` ([S_i, D] fp32 device tensors, or one such tensor), D <= 512, with the meaning of PCAEstimator.fit /
    get_components.  The moments are taken about the first chunk's column mean.  Raises if the eigen-solver does not converge."""
    if isinstance(chunks, torch.Tensor):
        chunks = (chunks,)
    state = None
    for x in chunks:
        state = H.pca_moments(x, x.mean(0) if state is None else None, state)
    if state is None:
        raise ValueError('fit_pca: no data')
    cov, mean, n = H.pca_covariance(state)
    evals, evecs, sweeps, converged = H.sym_eig(cov, max_sweeps=max_sweeps)
    if not converged:
        raise Eg3dHipError(f'fit_pca: the eigen-solver did not converge in {sweeps} sweeps on the {cov.shape[0]} x {cov.shape[0]} covariance of {n} rows')
    D = cov.shape[0]
    K = D if n_components is None else int(n_components)
    if not 1 <= K <= D:
        raise ValueError(f'fit_pca: n_components {K} outside 1..{D}')
    total_var = torch.diagonal(cov).double().sum()
    stdev = evals[:K].clamp_min(0).sqrt()       # the projected variance along an eigenvector is its eigenvalue
    return PCAResult(evecs[:K].contiguous(), stdev, (stdev.double().square() / total_var).float(), mean, float(total_var), n, sweeps, converged)


def fit_w_pca(G, n_samples: int = 100_000, n_components: int = 512, seed: int = 0, chunk: int = 8192) -> PCAResult:
    """pca_anlaysis.py: the PCA of n_samples mapped latents at the frontal camera."""
    return fit_pca(sample_w(G, n_samples, seed=seed, chunk=chunk), min(int(n_components), G.w_dim))


def save_components(path: str, result_or_array) -> None:
    """[K, D] float32 .npy, the format of the reference's ganspace/pca_comp/*.npy."""
    a = result_or_array.components if isinstance(result_or_array, PCAResult) else result_or_array
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError(f'save_components: [K, D] components, got {a.shape}')
    with open(path, 'wb') as fh:                 # (np.save(path) would append '.npy' to other suffixes)
        np.save(fh, a)


def load_components(path: str) -> np.ndarray:
    a = np.load(path)
    if a.ndim != 2:
        raise ValueError(f'load_components: {path} holds {a.shape}, expected [K, D]')
    return np.ascontiguousarray(a, dtype=np.float32)


def edit_directions(components, idx_comp: int, start_layer: int = 0, layer_num: int = 12, edit_power: float = 1.0, num_imgs: int = 5,
                    num_ws: int = 14) -> torch.Tensor:
    """[num_imgs, num_ws, D] (on the components' device): row i is zero except for layers start_layer .. start_layer + layer_num - 1, which hold
    (-edit_power + 2 edit_power i / (num_imgs - 1)) * components[idx_comp] (run_ganspace.py:31-36)."""
    if start_layer < 0 or layer_num < 0 or start_layer + layer_num > num_ws:
        raise ValueError(f'edit_directions: layers {start_layer} .. {start_layer + layer_num - 1} do not fit {num_ws} layers')
    if num_imgs < 2:
        raise ValueError(f'edit_directions: at least two images span -edit_power .. edit_power, got {num_imgs}')
    comp = torch.as_tensor(components, dtype=torch.float32)
    out = torch.zeros((num_imgs, num_ws, comp.shape[1]), dtype=torch.float32, device=comp.device)
    for i in range(num_imgs):
        out[i, start_layer:start_layer + layer_num] = comp[idx_comp] * (-edit_power + ((2 * edit_power) / (num_imgs - 1)) * i)
    return out


def _edited(G, components, w, idx_comp, start_layer, layer_num, edit_power, num_imgs):
    w = torch.as_tensor(w, dtype=torch.float32)
    if w.dim() == 2:
        w = w.unsqueeze(0)
    if not w.is_cuda:
        raise Eg3dHipError('ganspace edits render on an AMD GPU (cuda device); there is no CPU fallback')
    d = edit_directions(components, idx_comp, start_layer, layer_num, edit_power, num_imgs, num_ws=w.shape[1]).to(w.device)
    return d, w[:1] + d


@torch.no_grad()
def edit_ganspace(G, components, w, cam, idx_comp: int, start_layer: int = 0, layer_num: int = 12, edit_power: float = 1.0, num_imgs: int = 5,
                  synth_kwargs: Optional[dict] = None, with_depth: bool = False) -> dict:
    """run_ganspace.edit_ganspace: dict(images uint8 [num_imgs,H,W,3], grid uint8 [Ht,Wt,3] = make_grid(nrow 8, padding 2) of them, directions
    [num_imgs,num_ws,D], ws [num_imgs,num_ws,D] = w + directions).  One image per synthesis call, as the reference: every call has the signature
    of an ordinary single-image synthesis.  with_depth=True adds depth [num_imgs,1,h,w], the same renders' raw image_depth (what
    images.head_matte(depth=...) takes)."""
    directions, ws = _edited(G, components, w, idx_comp, start_layer, layer_num, edit_power, num_imgs)
    cam = torch.as_tensor(cam, dtype=torch.float32).reshape(1, 25).to(ws.device)
    kw = dict(synth_kwargs or {})
    rendered, depths = [], []
    for i in range(num_imgs):
        o = G.synthesis(ws[i:i + 1], cam, **kw)
        rendered.append(o['image'].float())
        if with_depth:
            depths.append(o['image_depth'].float())
    images = torch.stack([H.image_grid_u8(img, nrow=1, padding=0) for img in rendered])
    grid = H.image_grid_u8(torch.cat(rendered, 0), nrow=8, padding=2)
    out = dict(images=images, grid=grid, directions=directions, ws=ws)
    if with_depth:
        out['depth'] = torch.cat(depths, 0)
    return out


@torch.no_grad()
def edit_orbit(G, components, w, idx_comp: int, start_layer: int = 0, layer_num: int = 12, edit_power: float = 1.0, num_imgs: int = 5,
               num_frames: int = 240, cameras: Optional[torch.Tensor] = None, synth_kwargs: Optional[dict] = None) -> torch.Tensor:
    """uint8 [num_imgs, num_frames, H, W, 3]: inference.render_orbit of every edited latent, through the same conversion."""
    from .inference import render_orbit
    _, ws = _edited(G, components, w, idx_comp, start_layer, layer_num, edit_power, num_imgs)
    kw = dict(synth_kwargs or {})
    if kw.pop('noise_mode', 'const') != 'const':
        raise ValueError("edit_orbit: render_orbit renders with noise_mode='const'")
    rows = []
    for i in range(num_imgs):
        frames = render_orbit(G, ws[i:i + 1], num_frames=num_frames, cameras=cameras, **kw)
        rows.append(torch.stack([H.image_grid_u8(f.float().unsqueeze(0), nrow=1, padding=0) for f in frames]))
    return torch.stack(rows)
