"""What a workspace holds before a call, for tests/test_gpu_workspace_states.py: three byte patterns and "stale", the bytes
another stage left in the shared buffer.  droplets.py and density.py allocate ONE buffer per batch and run every stage of
every image at its base, so the state a stage finds is the first bytes of what the stage before it wrote at another geometry;
prepare() copies exactly those bytes into a view of exactly the size the stage asks for."""
import numpy as np
import torch

PATTERNS = {"zero": 0x00, "ones": 0xFF, "a5": 0xA5}
STATES = tuple(PATTERNS) + ("stale",)


def fit_bytes(src, nbytes):
    """The first nbytes of the uint8 tensor `src`, `src` repeated where it is shorter (a stage whose workspace is larger than
    the one before it: the rest of the shared buffer holds what earlier images left, here the same bytes again)."""
    assert src.dtype == torch.uint8 and src.dim() == 1 and (src.numel() > 0 or nbytes == 0)
    if src.numel() >= nbytes:
        return src[:nbytes]
    return src.repeat((nbytes + src.numel() - 1) // src.numel())[:nbytes]


def prepare(ws, state, stale=None):
    """Fill the view of the Canaried `ws` (tests/image_canaries.py) for `state`; the guards around it keep their canaries."""
    if state == "stale":
        ws.u8.copy_(fit_bytes(stale, ws.nbytes))
    else:
        ws.u8.fill_(PATTERNS[state])
    return ws


def holds(ws, state, stale=None):
    """True while the view still holds exactly what prepare() put there."""
    want = fit_bytes(stale, ws.nbytes) if state == "stale" else torch.full_like(ws.u8, PATTERNS[state])
    return bool(torch.equal(ws.u8, want.to(ws.u8.device)))


def droplet_table(mask):
    """(area int32 [n], sum of rows int64 [n], sum of columns int64 [n]) of the 4-connected components of `mask` in label order:
    what unetdc_ccl_stats with min_area = 1 hands unetdc_density_maps."""
    from scipy import ndimage
    from utils import droplet_match as dm
    lab = ndimage.label(mask)[0]
    a, sy, sx = dm.label_sums(lab)
    return a.astype(np.int32), sy, sx
