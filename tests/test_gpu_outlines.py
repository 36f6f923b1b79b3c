"""GPU: droplet outlines as polygons (csrc/outlines.hip) through the C ABI against the sequential crack
follower utils/droplet_outlines.outlines_numpy, integer for integer and vertex for vertex, at the smallest sizes where the
kernels can go wrong; then outlines.label_outlines_batch and the script's flag.  Every output and the workspace sit between
canaries.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

from tests.image_canaries import Canaried, canaried_like
from tests.test_outlines_cpu import known_map, known_shapes, random_labels
from tests.workspace_states import holds, prepare
from utils import droplet_outlines as do

pytestmark = pytest.mark.gpu

Q, F = do.QUANTITIES, do.CONTOUR_FIELDS
NQ, NF = len(Q), len(F)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def exact_rooms(ref):
    c = ref["contours"]
    return {"max_cracks": int(c["length"].sum()), "max_len": int(c["length"].max(initial=0)), "max_contours": len(c["label"]),
            "max_vertices": len(ref["x"])}


def device_outlines(lab, max_out, rooms, state=None, stale=None):
    """unetdc_label_outlines -> (record as outlines_numpy's, cut to the rooms; needed [4]; the views ws, contours, vx, vy)."""
    from unet_dc_segmentation_amd import _lib
    h, w = lab.shape
    mc, ml, mk, mv = (rooms[k] for k in ("max_cracks", "max_len", "max_contours", "max_vertices"))
    need = _lib.load().unetdc_label_outlines_workspace(h, w, max_out, mc)
    assert need > 0
    src = canaried_like(np.array(lab, dtype=np.int32))
    ws, out, cont = Canaried(need, align=8), Canaried(NQ * max_out * 8, align=8), Canaried(NF * mk * 8, align=8)
    vx, vy, cnt = Canaried(4 * mv, align=4), Canaried(4 * mv, align=4), Canaried(16, align=4)
    if state is not None:
        prepare(ws, state, stale)
    _lib.call("unetdc_label_outlines", src.ptr, max_out, h, w, ml, ws.ptr, need, out.ptr if max_out else None, cont.ptr if mk else None, mk,
              vx.ptr if mv else None, vy.ptr if mv else None, mv, mc, cnt.ptr, _stream())
    torch.cuda.synchronize()
    for v in (src, ws, out, cont, vx, vy, cnt):
        v.check()
    assert np.array_equal(src.numpy(np.int32, h, w), lab)
    needed = cnt.numpy(np.int32, 4).astype(np.int64)
    rows, table = out.numpy(np.int64, NQ, max_out), cont.numpy(np.int64, NF, mk)
    nc, nv = min(int(needed[1]), mk), min(int(needed[2]), mv)
    rec = {"rows": {q: rows[j] for j, q in enumerate(Q)}, "contours": {f: table[j, :nc] for j, f in enumerate(F)},
           "x": vx.numpy(np.int32, mv)[:nv], "y": vy.numpy(np.int32, mv)[:nv]}
    return rec, needed, (ws, cont, vx, vy)


def assert_equal(rec, ref):
    for q in Q:
        assert rec["rows"][q].dtype == np.int64 and np.array_equal(rec["rows"][q], ref["rows"][q]), (q, rec["rows"][q], ref["rows"][q])
    for f in F:
        assert np.array_equal(rec["contours"][f], ref["contours"][f]), (f, rec["contours"][f], ref["contours"][f])
    assert rec["x"].dtype == np.int32 and np.array_equal(rec["x"], ref["x"]) and np.array_equal(rec["y"], ref["y"])


def serpentine():
    """96 x 130, one label: every other row full, joined alternately at the right and the left end: one contour of 2 A + 2 cracks."""
    lab = np.zeros((96, 130), np.int32)
    lab[0::2] = 1
    lab[1::4, 129] = 1
    lab[3::4, 0] = 1
    return lab


def checkerboard():
    return (np.add.outer(np.arange(16), np.arange(16)) % 2 == 0).astype(np.int32)


def fixtures():
    three = random_labels(37, 53, seed=11)
    return {"known 16x48": known_map(), "1x1": np.ones((1, 1), np.int32), "1x64": np.ones((1, 64), np.int32),
            "64x1": np.ones((64, 1), np.int32), "37x53 full": np.full((37, 53), 2, np.int32), "16x16 checkerboard": checkerboard(),
            "37x53 random": three, "disc": known_shapes()["disc"][0], "96x130 serpentine": serpentine()}


FIXTURES = fixtures()
_refs = {}


def ref_of(name, max_out=None):
    """The follower's answer, computed once per (fixture, capacity) and shared."""
    max_out = int(FIXTURES[name].max()) if max_out is None else max_out
    if (name, max_out) not in _refs:
        ref = _refs[name, max_out] = do.outlines_numpy(FIXTURES[name], max_out)
        for v in (*ref["rows"].values(), *ref["contours"].values(), ref["x"], ref["y"]):
            v.setflags(write=False)
    return _refs[name, max_out]


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixtures_equal_the_follower(name):
    lab, ref = FIXTURES[name], ref_of(name)
    rooms = exact_rooms(ref)
    rec, needed, _ = device_outlines(lab, int(lab.max()), rooms)
    assert needed.tolist() == [rooms["max_cracks"], rooms["max_contours"], rooms["max_vertices"], 0]
    assert_equal(rec, ref)
    again, _, _ = device_outlines(lab, int(lab.max()), rooms, state="a5")       # two runs: the same bytes
    for part in ("rows", "contours"):
        assert all(again[part][k].tobytes() == rec[part][k].tobytes() for k in rec[part])
    assert again["x"].tobytes() == rec["x"].tobytes() and again["y"].tobytes() == rec["y"].tobytes()
    if name == "16x16 checkerboard":
        assert rec["rows"]["no"].tolist() == [128] and rec["rows"]["nh"].tolist() == [0] and rec["rows"]["E"].tolist() == [512]
    if name == "37x53 full":
        assert [rec["rows"][q].tolist() for q in Q] == [[0, 180], [0, 1], [0, 0], [0, 4], [0, 2 * 37 * 53], [0, 2 * 37 * 53]]
    if name == "96x130 serpentine":
        assert len(rec["contours"]["label"]) == 1 and rec["contours"]["length"][0] == 2 * int(lab.sum()) + 2 > 4096
    if name == "known 16x48":
        want = [v for n, (_, cs, _) in known_shapes().items() if n != "disc" for k in sorted(cs) for v in cs[k]]
        got = sorted(zip(rec["contours"]["label"].tolist(), rec["contours"]["length"].tolist(), rec["contours"]["S2"].tolist(),
                         rec["contours"]["nv"].tolist()), key=lambda t: t[0])
        assert [g[1:] for g in got] == [c[1:] for c in want]


def test_a_contour_longer_than_max_len_is_never_returned_in_pieces():
    name = "96x130 serpentine"
    lab, ref = FIXTURES[name], ref_of(name)
    rooms = exact_rooms(ref)
    for short in (rooms["max_len"] - 1, 4096, 5, 1, 0):      # below the length in the same number of rounds, and in fewer
        rec, needed, (_, cont, vx, vy) = device_outlines(lab, 1, {**rooms, "max_len": short})
        assert needed.tolist() == [rooms["max_cracks"], 0, 0, 1]
        assert cont.untouched() and vx.untouched() and vy.untouched() and not any(rec["rows"][q].any() for q in Q)
    rec, needed, _ = device_outlines(lab, 1, {**rooms, "max_len": rooms["max_len"] + 1000})
    assert needed[3] == 0
    assert_equal(rec, ref)


def test_batch_retries_a_contour_longer_than_its_room():
    from unet_dc_segmentation_amd import _lib
    from unet_dc_segmentation_amd.outlines import ROOM_KEYS, label_outlines_batch, rooms_for
    names = ["96x130 serpentine", "37x53 random"]
    labs = [torch.from_numpy(FIXTURES[n]).cuda() for n in names]
    areas = [np.bincount(FIXTURES[n].ravel(), minlength=int(FIXTURES[n].max()) + 1)[1:] for n in names]
    calls = []
    real = _lib.call
    try:
        _lib.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        small = [{**exact_rooms(ref_of(names[0])), "max_len": 4096}, exact_rooms(ref_of(names[1]))]
        recs = label_outlines_batch(labs, areas, rooms=small)
        assert calls == ["unetdc_label_outlines"] * 3        # the batch, then the serpentine alone
        calls.clear()
        computed = label_outlines_batch(labs, areas, connected=False)
        assert calls == ["unetdc_label_outlines"] * 2
        calls.clear()
        tight = label_outlines_batch(labs, areas, rooms={k: 7 for k in ROOM_KEYS})
        assert calls == ["unetdc_label_outlines"] * 4
    finally:
        _lib.call = real
    for got in (recs, computed, tight):
        for rec, n in zip(got, names):
            assert sorted(rec) == ["contours", "rows", "x", "y"]
            assert_equal(rec, ref_of(n))
    r = rooms_for(areas[0])                                  # the serpentine meets the bound of a connected label
    assert r["max_cracks"] == r["max_len"] == exact_rooms(ref_of(names[0]))["max_cracks"]
    with pytest.raises(_lib.UnetdcError):
        label_outlines_batch([labs[0].long()], areas[:1])
    with pytest.raises(_lib.UnetdcError):
        label_outlines_batch([labs[0].cpu()], areas[:1])
    with pytest.raises(_lib.UnetdcError):
        label_outlines_batch(labs, areas[:1])
    assert label_outlines_batch([], []) == []


@pytest.mark.parametrize("short", ["max_cracks", "max_contours", "max_vertices"])
def test_each_room_one_below_what_is_needed(short):
    name = "37x53 random"
    lab, ref = FIXTURES[name], ref_of(name)
    rooms = exact_rooms(ref)
    rec, needed, (_, cont, vx, vy) = device_outlines(lab, 3, {**rooms, short: rooms[short] - 1})     # the canaries held
    if short == "max_cracks":                                # only needed[0] means anything
        assert needed.tolist() == [rooms["max_cracks"], 0, 0, 0]
        assert cont.untouched() and vx.untouched() and vy.untouched() and not any(rec["rows"][q].any() for q in Q)
        return
    assert needed.tolist() == [rooms["max_cracks"], rooms["max_contours"], rooms["max_vertices"], 0]
    for q in Q:                                              # the per-label rows are complete
        assert np.array_equal(rec["rows"][q], ref["rows"][q]), q
    nc, nv = len(rec["contours"]["label"]), len(rec["x"])
    assert (nc, nv) == ((rooms["max_contours"] - 1, rooms["max_vertices"]) if short == "max_contours" else (rooms["max_contours"], rooms["max_vertices"] - 1))
    for f in F:                                              # what fits is what the follower lists first
        assert np.array_equal(rec["contours"][f], ref["contours"][f][:nc]), f
    assert np.array_equal(rec["x"], ref["x"][:nv]) and np.array_equal(rec["y"], ref["y"][:nv])


def test_zero_rooms_and_capacities():
    name = "37x53 random"
    lab, full = FIXTURES[name], exact_rooms(ref_of(name))
    rec, needed, _ = device_outlines(lab, 3, {**full, "max_contours": 0, "max_vertices": 0})
    assert needed.tolist() == [full["max_cracks"], full["max_contours"], full["max_vertices"], 0]
    assert all(np.array_equal(rec["rows"][q], ref_of(name)["rows"][q]) for q in Q)
    rec, needed, _ = device_outlines(lab, 3, {k: 0 for k in full})
    assert needed.tolist() == [full["max_cracks"], 0, 0, 0]
    ref2 = ref_of(name, 2)                                   # a capacity below the largest label present: 3 is skipped, and not k
    rec, needed, _ = device_outlines(lab, 2, exact_rooms(ref2))
    assert needed[0] == exact_rooms(ref2)["max_cracks"] < full["max_cracks"]
    assert_equal(rec, ref2)
    ref5 = ref_of(name, 5)                                   # and above it: two numbers without pixels
    rec, _, _ = device_outlines(lab, 5, exact_rooms(ref5))
    assert_equal(rec, ref5)
    assert not any(rec["rows"][q][3:].any() for q in Q)
    rec, needed, _ = device_outlines(lab, 0, {k: 0 for k in full})
    assert needed.tolist() == [0, 0, 0, 0] and all(rec["rows"][q].size == 0 for q in Q)
    rec, needed, _ = device_outlines(np.zeros((5, 7), np.int32), 3, {"max_cracks": 9, "max_len": 9, "max_contours": 2, "max_vertices": 9})
    assert needed.tolist() == [0, 0, 0, 0] and not any(rec["rows"][q].any() for q in Q)


@pytest.mark.parametrize("state", ["ones", "stale"])
def test_workspace_may_hold_anything(state):
    name = "37x53 random"
    lab, ref = FIXTURES[name], ref_of(name)
    stale = None
    if state == "stale":                                     # a second trip: what the stage left after a larger image
        big = "96x130 serpentine"
        stale = device_outlines(FIXTURES[big], 1, exact_rooms(ref_of(big)))[2][0].u8.clone()
    rec, needed, (ws, *_) = device_outlines(lab, 3, exact_rooms(ref), state=state, stale=stale)
    assert needed[3] == 0 and not holds(ws, state, stale)
    assert_equal(rec, ref)
    rec, needed, _ = device_outlines(lab, 3, {**exact_rooms(ref), "max_cracks": 5}, state=state, stale=stale)
    assert needed.tolist() == [exact_rooms(ref)["max_cracks"], 0, 0, 0]


# ---- behind the droplet stage --------------------------------------------------------------------------------------------------------

def batch_inputs():
    from tests.test_split_cpu import noise_mask
    hws = [(120, 160), (97, 131)]
    p = np.stack([np.where(noise_mask(64, 80, seed=70 + i, sigma=2.0, frac=0.35) > 0, 0.8, 0.1).astype(np.float32) for i in range(2)])
    return hws, p


def test_behind_mask_and_droplets_batch():
    """Two images of different sizes, split droplets: the record equals the follower's on the label map the stage returned, and
    the droplet stage's own launches are the same with and without the outlines behind them."""
    from unet_dc_segmentation_amd import droplets as D
    from unet_dc_segmentation_amd.outlines import label_outlines_batch
    hws, p = batch_inputs()
    probs = torch.from_numpy(p).cuda()
    names = []
    real = D._lib.call
    try:
        D._lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
        out = D.mask_and_droplets_batch(probs, 0.5, hws, 2, split_depth=2.0, return_labels=True)
        parent = list(names)
        recs = label_outlines_batch([d.labels for d in out], [d.area for d in out], connected=False)
        assert names == parent + ["unetdc_label_outlines"] * 2 and "unetdc_label_outlines" not in parent
        names.clear()
        D.mask_and_droplets_batch(probs, 0.5, hws, 2, split_depth=2.0, return_labels=True)
        assert names == parent
    finally:
        D._lib.call = real
    assert min(len(d.area) for d in out) > 4
    for d, rec in zip(out, recs):
        lab = d.labels.cpu().numpy()
        want = do.outlines_numpy(lab, len(d.area))
        assert_equal(rec, want)
        cols, ref = do.outline_columns(rec, d.area), do.outline_columns(want, np.bincount(lab.ravel(), minlength=len(d.area) + 1)[1:])
        assert list(cols) == list(ref) and all(cols[k].tobytes() == ref[k].tobytes() for k in ref)


def test_cli_device_equals_cpu_path_and_adds_only_its_launches(tmp_path, monkeypatch):
    """quantify_droplets_batch.py --outlines on the device against its CPU path on the synthetic set (the network is the exact
    stand-in of tests/test_tta_cpu.py): identical files.  Without the flag the run's launches are the parent's: no
    unetdc_label_outlines; with it, the same sequence plus one unetdc_label_outlines per image."""
    import quantify_droplets_batch as q
    from tests.test_confidence_cpu import files, run_script
    from unet_dc_segmentation_amd import _lib
    assert q.DEVICE == "cuda"
    sizes = ((96, 96), (80, 112), (64, 64))
    names = []
    real = _lib.call
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
        off = run_script(tmp_path, mp, "off", ["--split_touching"], device="cuda", sizes=sizes)
        parent = list(names)
        names.clear()
        dev = run_script(tmp_path, mp, "dev", ["--split_touching", "--outlines"], device="cuda", sizes=sizes)
    assert "unetdc_label_outlines" not in parent and names.count("unetdc_label_outlines") == 3
    assert [n for n in names if n != "unetdc_label_outlines"] == parent
    cpu = run_script(tmp_path, monkeypatch, "cpu", ["--split_touching", "--outlines"], device="cpu", sizes=sizes)
    assert files(dev) == files(cpu) and set(files(dev)) - set(files(off)) == {"outlines_coco.json"} | {f"outlines/im{i}.geojson" for i in range(3)}
    for f in files(dev):
        assert (dev / f).read_bytes() == (cpu / f).read_bytes(), f
    plain = run_script(tmp_path, monkeypatch, "plain", ["--outlines"], device="cuda", sizes=sizes)          # asks for the label map itself
    plain_cpu = run_script(tmp_path, monkeypatch, "plain_cpu", ["--outlines"], device="cpu", sizes=sizes)
    for f in files(plain):
        assert (plain / f).read_bytes() == (plain_cpu / f).read_bytes(), f
