"""The yardstick of the diffusion filter's tests: the recurrence of preprocess.anisotropic_diffusion evaluated in float64
throughout (arrays, kappa and gamma), started from the float32-rounded image.  The float32 implementations (the NumPy one on
the host, the kernel on the GPU) are roundings of this one recurrence; their distances to it are their own rounding errors."""
import numpy as np


def diffusion_f64(img, niter=1, kappa=50, gamma=0.1, option=1):
    out = np.asarray(img, dtype=np.float32).astype(np.float64)
    assert out.ndim == 2 and option in (1, 2)
    kappa, gamma = np.float64(kappa), np.float64(gamma)
    for _ in range(int(niter)):
        ds, de = np.zeros_like(out), np.zeros_like(out)
        ds[:-1, :] = out[1:, :] - out[:-1, :]                  # forward differences, 0 at the far border
        de[:, :-1] = out[:, 1:] - out[:, :-1]
        if option == 1:
            fs, fe = np.exp(-(ds / kappa) ** 2) * ds, np.exp(-(de / kappa) ** 2) * de
        else:
            fs, fe = ds / (1.0 + (ds / kappa) ** 2), de / (1.0 + (de / kappa) ** 2)
        div = fs + fe
        div[1:, :] -= fs[:-1, :]                               # backward difference of the flux
        div[:, 1:] -= fe[:, :-1]
        out = out + gamma * div
    assert out.dtype == np.float64
    return out


def contact_like(rng, shape):
    """a non-negative image with the loader's value range: log1p of uniform noise"""
    return np.log1p(rng.random(shape) * 6.0)


DIFFUSION_CASES = [(5, 50.0, 1), (10, 50.0, 1), (3, 0.05, 1)]           # (niter, kappa, option)
DIFFUSION_SHAPES = [(1, 64), (64, 1), (97, 131), (1000, 1000)]
