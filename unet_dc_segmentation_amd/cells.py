"""Droplets per cell on the HIP device (csrc/cells.hip): ``nearest_label`` turns a label map of nuclei into
their territories (every pixel gets the label of the nearest nucleus pixel and its exact squared distance), ``cell_table``
reduces a droplet label map against a cell label map.  In the quantification flow the table is the ``cells`` stage of
``droplets.mask_and_droplets_batch``, which takes one ``CellMap`` per image.

The definitions are those of ``utils/droplet_cells.py``, whose numpy form is the path of CPU tensors and the yardstick of the
kernels.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
from utils import droplet_cells

from . import _lib

N_DROPLET_ROWS, N_CELL_ROWS = len(droplet_cells.DROPLET_QUANTITIES), len(droplet_cells.CELL_QUANTITIES)   # UNETDC_CELL_*_QUANTITIES


class CellMap(NamedTuple):
    """One image's cells for the droplet stage: label, int32 [oh, ow] on the device (cells 1..max_label, anything else is
    background); d2, int32 [oh, ow] or None: the squared distance to the nearest nucleus pixel (nearest_label's second plane)."""
    label: torch.Tensor
    max_label: int
    d2: torch.Tensor | None = None


def _check_map(label, what):
    if not torch.is_tensor(label) or label.dim() != 2 or label.dtype != torch.int32:
        raise _lib.UnetdcError(f"{what}: the label map must be an int32 [h, w] tensor")


def nearest_label(label, max_label, radius=0, workspace=None):
    """label: int32 [h, w], seeds 1..max_label -> (territory label int32 [h, w], squared distance int32 [h, w]): per pixel the
    label of the nearest seed pixel (the smallest label among equidistant ones) and the exact squared distance to it; with a
    radius > 0 the label is 0 beyond it.  On the HIP device: two launches on the current stream, nothing waits (workspace: a
    uint8 tensor to use when it is large enough); CPU tensors take utils.droplet_cells.nearest_label_numpy."""
    _check_map(label, "nearest_label")
    try:
        radius = droplet_cells.check_radius(radius)
    except (ValueError, TypeError) as e:
        raise _lib.UnetdcError(str(e)) from None
    max_label = int(max_label)
    if not label.is_cuda:
        try:
            out = droplet_cells.nearest_label_numpy(label.numpy(), max_label, radius)
        except ValueError as e:
            raise _lib.UnetdcError(str(e)) from None
        return tuple(torch.from_numpy(a) for a in out)
    label = label.contiguous()
    h, w = label.shape
    nbytes = int(_lib.load().unetdc_label_nearest_workspace(h, w)) if h and w else 0
    if nbytes == 0 or max_label < 0:
        raise _lib.UnetdcError(f"nearest_label: {[h, w]} outside the limits (sides 1..16384, a non-negative label limit)")
    if (workspace is None or workspace.dtype != torch.uint8 or workspace.device != label.device or workspace.numel() < nbytes
            or workspace.data_ptr() % 4):
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=label.device)
    out_label, out_d2 = torch.empty_like(label), torch.empty_like(label)
    _lib.call("unetdc_label_nearest", label.data_ptr(), max_label, h, w, radius, workspace.data_ptr(), workspace.numel(),
              out_label.data_ptr(), out_d2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out_label, out_d2


def cell_table(droplet_label, max_droplet, cell_label, max_cell, d2=None, max_pairs=None):
    """Two int32 [h, w] label maps on the HIP device (and optionally the d2 plane) -> the record of
    utils.droplet_cells.cells_record, host arrays.  max_pairs: the room for (droplet, cell) pairs of the first launch (default
    1 << 14); a map with more is run again with the room it needs.  One host wait per launch."""
    for t in (droplet_label, cell_label) + (() if d2 is None else (d2,)):
        _check_map(t, "cell_table")
        if not t.is_cuda or t.shape != droplet_label.shape:
            raise _lib.UnetdcError("cell_table: the maps must lie on the HIP device and be of one size")
    lib, (h, w), dev = _lib.load(), droplet_label.shape, droplet_label.device
    max_droplet, max_cell = int(max_droplet), int(max_cell)
    room = int(min(1 << 14 if max_pairs is None else max_pairs, h * w))
    maps = [t.contiguous() for t in (droplet_label, cell_label)] + [None if d2 is None else d2.contiguous()]
    while True:
        nbytes = int(lib.unetdc_cell_table_workspace(h, w, max_droplet, max_cell, room)) if h and w else 0
        if nbytes == 0:
            raise _lib.UnetdcError("cell_table: outside the limits (sides 1..16384, non-negative label and pair limits)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        needed = torch.zeros(1, dtype=torch.int32, device=dev)
        out_d = torch.empty(N_DROPLET_ROWS, max_droplet, dtype=torch.int32, device=dev)
        out_c = torch.empty(N_CELL_ROWS, max_cell, dtype=torch.int64, device=dev)
        _lib.call("unetdc_cell_table", maps[0].data_ptr(), max_droplet, maps[1].data_ptr(), max_cell,
                  None if maps[2] is None else maps[2].data_ptr(), h, w, ws.data_ptr(), nbytes, needed.data_ptr(), room,
                  out_d.data_ptr() if max_droplet else None, out_c.data_ptr() if max_cell else None,
                  torch.cuda.current_stream().cuda_stream)
        n = int(needed.item())
        if n <= room:
            return droplet_cells.make_record(out_d.cpu().numpy().astype(np.int64), out_c.cpu().numpy(), d2 is not None)
        room = int(min(max(2 * room, 1), h * w))
