"""CPU tests of adaptive sampling's host side (no GPU needed): the entry points are declared in the header, exported by both builds of the
library and prototyped in rtamd/abi.py; null handles are refused without a HIP call; the CLI documents and checks --adaptive; the block
grid's arithmetic; and the float64 model of the two-image error estimate (rt_mi355x.h) that tests/test_gpu_adaptive.py holds the library
to, on hand-made arrays, with its vectorised form (the one tests/test_gpu_continuations_full_size.py uses at full frame size) equal to it."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

from rtamd import abi

REPO = Path(__file__).resolve().parent.parent
EXE = REPO / "sycl-ray-tracer_amd" / "host" / "build" / "raytracer"
ENTRY_POINTS = ["rt_renderer_block_grid", "rt_render_frame_continue_blocks", "rt_render_frame_continue_blocks_device", "rt_renderer_block_samples",
                "rt_renderer_adapt", "rt_render_frame_continue_adaptive", "rt_render_frame_continue_adaptive_device", "rt_renderer_block_errors"]
EPS = 1e-4


def block_grid(width, local_rows):
    """(blocks_x, blocks_y) of a tile: 8x8 blocks, the right and bottom ones ragged."""
    return (width + 7) // 8, (local_rows + 7) // 8


def block_errors_model(I, before, counts, eps=EPS):
    """e_B in float64 (rt_mi355x.h). I: (rows, W, 3) linear image of the current state (the last image returned, squared); before: (by, bx,
    rows, W, >= 3) per block the image it had before its last render, in sqrt space as returned (A = its square; all zero = no snapshot);
    counts: (by, bx). Returns (by, bx), +inf where a block has no snapshot."""
    by, bx = counts.shape
    rows, w = I.shape[:2]
    out = np.full((by, bx), np.inf)
    for y in range(by):
        for x in range(bx):
            A = before[y, x].astype(np.float64)[y * 8:y * 8 + 8, x * 8:x * 8 + 8, :3] ** 2
            if not A.any() and not before[y, x][..., 3].any():
                continue  # never rendered since the frame: no snapshot
            Ib = I[y * 8:y * 8 + 8, x * 8:x * 8 + 8, :3]
            e = np.abs(Ib - A).sum(-1) / np.sqrt(eps + Ib.sum(-1))
            out[y, x] = e.mean()
    return out


def block_index_map(rows, w):
    """(rows, w) map of every pixel's block index, tile-local row-major."""
    bx = (w + 7) // 8
    return (np.arange(rows)[:, None] // 8) * bx + np.arange(w)[None, :] // 8


def block_errors_vec(I, before, counts, has_snap, eps=EPS):
    """block_errors_model without a whole image per block. I: (rows, W, 3) linear image of the current state; before: (rows, W, >= 3) every
    pixel's image as of its block's last render, in sqrt space as returned; counts: (by, bx); has_snap: (by, bx) bool, whether the block has a
    snapshot. Returns (by, bx) float64, +inf where a block has none."""
    by, bx = counts.shape
    rows, w = I.shape[:2]
    A = before[..., :3].astype(np.float64) ** 2
    I = I[..., :3].astype(np.float64)
    e = np.abs(I - A).sum(-1) / np.sqrt(eps + I.sum(-1))
    idx = block_index_map(rows, w).reshape(-1)
    n_in = np.bincount(idx, minlength=by * bx)
    out = np.bincount(idx, weights=e.reshape(-1), minlength=by * bx) / np.maximum(n_in, 1)
    out[~np.asarray(has_snap, bool).reshape(-1)] = np.inf
    return out.reshape(by, bx)


def test_entry_points_are_declared_exported_and_prototyped(rtlib, devlib):
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "rt_mi355x.h").read_text(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"{name} is not declared in include/rt_mi355x.h"
        assert hasattr(rtlib, name) and hasattr(devlib, name), f"{name} is not exported"
        assert name in abi.PROTOTYPES and abi.PROTOTYPES[name][0] is C.c_int
    assert re.search(r"RT_K_BLOCK_RESOLVE\s*=\s*13", text) and abi.KERNELS["block_resolve"] == 13 < abi.RT_K_COUNT


def test_null_handles_are_refused_without_a_device(rtlib):
    n = C.c_uint32(7)
    st = abi.rt_stats()
    lst = (C.c_uint32 * 2)(0, 1)
    assert rtlib.rt_renderer_block_grid(None, C.byref(n), C.byref(n)) == abi.RT_ERR_INVALID
    assert rtlib.rt_render_frame_continue_blocks(None, 1, lst, 2, None, None, C.byref(st)) == abi.RT_ERR_INVALID
    assert rtlib.rt_render_frame_continue_blocks_device(None, 1, lst, 2, None, None, None, C.byref(st)) == abi.RT_ERR_INVALID
    assert rtlib.rt_renderer_block_samples(None, lst) == abi.RT_ERR_INVALID
    assert rtlib.rt_renderer_adapt(None, 0.1, 0, lst, C.byref(n)) == abi.RT_ERR_INVALID
    assert rtlib.rt_render_frame_continue_adaptive(None, 1, 0.1, 0, None, None, C.byref(st), C.byref(n)) == abi.RT_ERR_INVALID
    assert rtlib.rt_render_frame_continue_adaptive_device(None, 1, 0.1, 0, None, None, None, C.byref(st), C.byref(n)) == abi.RT_ERR_INVALID
    assert rtlib.rt_renderer_block_errors(None, (C.c_float * 1)()) == abi.RT_ERR_INVALID
    assert n.value == 7 and b"null" in rtlib.rt_last_error()


def test_cli_documents_and_checks_the_adaptive_flags(tmp_path):
    help_text = subprocess.run([str(EXE), "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--adaptive" in help_text and "--min-samples" in help_text
    for args, code in ((["--adaptive", "-1"], 105), (["--adaptive", "x"], 105), (["--adaptive"], 106), (["--min-samples", "x"], 104)):
        p = subprocess.run([str(EXE), str(REPO / "assets" / "cube.glb")] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert p.returncode == code, (args, p.returncode, p.stdout, p.stderr)
        assert args[0] in p.stderr
        assert not (tmp_path / "out.png").exists()


def test_block_grid_arithmetic():
    assert block_grid(1920, 1080) == (240, 135)
    assert block_grid(61, 45) == (8, 6)
    assert block_grid(8, 4) == (1, 1)
    assert block_grid(24, 0) == (3, 0)
    assert block_grid(1920, 360) == (240, 45)  # rank 1 of 3 in 8-row strips of 1080 rows: 360 rows


def test_estimator_model_on_hand_made_arrays():
    """One 12 x 10 image, 2 x 2 blocks (ragged): a block equal to its snapshot has e_B 0; a known difference gives the formula's value; the
    ragged block averages over its pixels in the image only; a block without a snapshot is +inf."""
    rows, w = 10, 12
    I = np.full((rows, w, 3), 0.25)
    before = np.zeros((2, 2, rows, w, 4))
    counts = np.full((2, 2), 8, np.uint32)
    before[0, 0, ..., :3], before[0, 0, ..., 3] = 0.5, 1.0     # A = 0.25 = I
    before[0, 1, ..., :3], before[0, 1, ..., 3] = np.sqrt(0.36), 1.0  # A = 0.36
    before[1, 0, ..., :3], before[1, 0, ..., 3] = 0.5, 1.0
    before[1, 0, 9, 3, :3] = 0.0                                # one pixel of the ragged bottom-left block: A = 0
    e = block_errors_model(I, before, counts)
    assert e[0, 0] == 0.0
    np.testing.assert_allclose(e[0, 1], 3 * 0.11 / np.sqrt(EPS + 0.75), rtol=1e-12)
    np.testing.assert_allclose(e[1, 0], (3 * 0.25 / np.sqrt(EPS + 0.75)) / 16, rtol=1e-12)  # 8 x 2 pixels in the image
    assert np.isinf(e[1, 1])


def _per_pixel_snapshots(before):
    """The per-pixel image of each block's snapshot and the snapshot flags, from block_errors_model's per-block images."""
    by, bx, rows, w = before.shape[:4]
    idx = block_index_map(rows, w)
    img = before.reshape(by * bx, rows, w, -1)[idx, np.arange(rows)[:, None], np.arange(w)[None, :]]
    has = np.array([[before[y, x].any() for x in range(bx)] for y in range(by)])
    return img, has


def test_vectorised_estimator_equals_the_model():
    """block_errors_vec against block_errors_model: the hand-made arrays above, then random images with ragged right and bottom blocks,
    blocks without a snapshot, snapshots equal to the image and all-black pixels (A = I = 0: e_p = 0, the eps keeps the root positive)."""
    rows, w = 10, 12
    I = np.full((rows, w, 3), 0.25)
    before = np.zeros((2, 2, rows, w, 4))
    before[0, 0, ..., :3], before[0, 0, ..., 3] = 0.5, 1.0
    before[0, 1, ..., :3], before[0, 1, ..., 3] = np.sqrt(0.36), 1.0
    before[1, 0, ..., :3], before[1, 0, ..., 3] = 0.5, 1.0
    before[1, 0, 9, 3, :3] = 0.0
    counts = np.full((2, 2), 8, np.uint32)
    img, has = _per_pixel_snapshots(before)
    vec, model = block_errors_vec(I, img, counts, has), block_errors_model(I, before, counts)
    assert (np.isinf(vec) == np.isinf(model)).all() and vec[0, 0] == 0.0
    np.testing.assert_allclose(vec[~np.isinf(vec)], model[~np.isinf(model)], rtol=1e-12, atol=0)  # (the two sum in different orders)
    rng = np.random.default_rng(5)
    for rows, w in ((8, 8), (9, 17), (21, 13), (24, 40), (1, 3), (31, 33)):
        bx, by = block_grid(w, rows)
        cur = rng.random((rows, w, 4)).astype(np.float32)
        cur[rng.random((rows, w)) < 0.1, :3] = 0.0
        I = cur[..., :3].astype(np.float64) ** 2
        before = np.zeros((by, bx, rows, w, 4), np.float32)
        counts = rng.integers(1, 100, (by, bx)).astype(np.uint32)
        snap = rng.random((by, bx)) < 0.7
        snap.reshape(-1)[0] = True
        for y in range(by):
            for x in range(bx):
                if snap[y, x]:
                    before[y, x] = cur if rng.random() < 0.2 else rng.random((rows, w, 4)).astype(np.float32)
                    before[y, x, ..., 3] = 1.0
        img, has = _per_pixel_snapshots(before)
        assert (has == snap).all()
        model = block_errors_model(I, before, counts)
        vec = block_errors_vec(I, img, counts, snap)
        assert (np.isinf(vec) == ~snap).all() and (np.isinf(model) == ~snap).all()
        np.testing.assert_allclose(vec[snap], model[snap], rtol=1e-12, atol=0)
