"""Scores and signals a network would never emit but a caller of the C API may pass, for the per-read feature kernels (remap, site mods, variants, events, poly
tail): what tests/test_features_hostile_gpu.py gives the operators and tests/test_remap.py / test_sitemods.py give the restatements.  Nothing here imports the
package; every matrix is a function of its arguments alone."""
import functools

import numpy as np

import remap_ref as R

SPARSE = ("nan 0.1%", "nan 5%", "-inf 0.1%", "-inf 5%", "+inf 0.1%")
STYLES = ("flat", "quantised") + SPARSE + ("nan block", "all nan", "all -inf", "all +inf", "+-3e38")
# the smallest shapes that reach the four kernel forms of remap at W in REMAP_BANDS: the window min(2 W + 1, L) is <= 64, <= 256, <= 1024 and > 1024
REMAP_SHAPES = ((64, 1), (65, 40), (300, 170), (300, 301), (400, 300), (1100, 1090))
REMAP_BANDS = (0, 5, 2048)


def form(L, W):
    """ffhip_debug_remap_form: the kernel form of a window of min(2 W + 1, L) cells (tests/test_features_hostile_gpu.py holds this to the library's)"""
    wd = min(2 * W + 1, L)
    return next((f for f, cells in enumerate((64, 256, 1024, 4608)) if wd <= cells), -1)


def base_scores(seed, N, nbase):
    """2 N(0, 1), float32: what every style is built on"""
    return (2.0 * np.random.default_rng(seed).standard_normal((N, 2 * nbase * (nbase + 1)))).astype(np.float32)


def styled(style, seed, N, nbase):
    """the base matrix of this seed in the given style; a sparse style and "nan block" leave every other entry as base_scores(seed, N, nbase) has it (site mods
    and variants: a path made from the base matrix stays a path of the styled one)"""
    T = base_scores(seed, N, nbase)
    rng = np.random.default_rng([seed, STYLES.index(style)])
    if style == "flat":
        return np.zeros_like(T)
    if style == "quantised":
        return (np.round(T * 4.0) / 4.0).astype(np.float32)
    if style in SPARSE:
        what, share = style.split()
        T[rng.random(T.shape) < float(share[:-1]) / 100.0] = np.float32(what)
        return T
    if style == "nan block":
        T[N // 2] = np.nan
        return T
    if style.startswith("all "):
        return np.full_like(T, np.float32(style.split()[1]))
    assert style == "+-3e38"
    return (np.sign(T) * np.float32(3e38)).astype(np.float32)


def remap_cases(shapes=REMAP_SHAPES):
    """(style, nbase, N, L, W, seed) of the sweep"""
    for N, L in shapes:
        for nbase in (4, 5):
            for k, style in enumerate(STYLES):
                for W in REMAP_BANDS:
                    yield style, nbase, N, L, W, 1000 * N + 10 * L + nbase + 100000 * k


def sequence(seed, L, nbase):
    """letters with runs of equal ones (the flip / flop coding)"""
    rng = np.random.default_rng([seed, 7])
    s = rng.integers(0, nbase, L).astype(np.uint8)
    rep = rng.random(L) < 0.3
    for i in range(1, L):
        if rep[i]:
            s[i] = s[i - 1]
    return s


@functools.lru_cache(maxsize=None)
def remap_reference(N, L):
    """{(style, nbase, W): (T, s, status, score, rm)} of one shape by remap_ref.remap_status, computed once"""
    out = {}
    for style, nbase, N_, L_, W, seed in remap_cases(((N, L),)):
        T, s = styled(style, seed, N, nbase), sequence(seed, L, nbase)
        out[style, nbase, W] = (T, s) + R.remap_status(T, s, nbase, W)
    return out
