"""CPU: the order-fixed BEV splat's contract as range_image.to_voxel_ordered_host states it, and the inputs of
tests/test_bev_ordered_gpu.py.

  statement   to_voxel_ordered_host against a literal Python loop over the votes in ascending id v = n * 8 + (dx * 4 + dy * 2 + dz), one
              fp32 addition per counted vote, bit for bit; and within splat_bounds (tests/test_lidar_exact.py) of the fp64 reference
  inputs      the inputs can tell orders apart: summing each cell in descending v instead gives other bits in at least 10 cells of every
              bev_input case, and in at least half of the occupied cells of the crowded input
  crowded     crowded_input (used by the GPU tests) is what its docstring says: chunks spanned, a cell fed by every chunk, a ragged tail
  wiring      the command line takes --bev-ordered and keeps its refusal without it

The helpers are tests/bev_util.py's and tests/test_lidar_exact.py's, imported."""
import functools

import numpy as np
import pytest
import torch

from rangeldm_amd import train_vae as CLI
from tests import bev_util as BU
from tests.test_lidar_exact import FiveSteep, bits

F = np.float32
GRID_CASES = pytest.mark.parametrize("grid,pc_range", BU.SPLAT_GRIDS, ids=BU.SPLAT_IDS)
MODE_CASES = pytest.mark.parametrize("mode", BU.MODES)

# csrc/lidar.hip: the radix sort's unit is a chunk of ORD_CHUNK = 1024 consecutive vote positions, owned by one wave, walked in rounds
# of 64; a cell's segment of more than ORD_SHORT = 16 votes is read by the whole wave, 64 votes a load.
ORD_CHUNK, ORD_ROUND, ORD_SHORT = 1024, 64, 16

# The crowded input: W = 509 columns of the five-beam steep sensor.  An image holds 8 * 509 * 5 = 20 360 vote positions = 19 full
# chunks and one of 904 positions (20 chunks: more than three sort units); 20 360 = 318 * 64 + 8, so the last round of the last chunk
# has 8 live lanes; neither the chunk nor the round divides the count.
CROWD_W, CROWD_B = 509, 3
CROWD_GRID = ((1, 4, 4), (-4., -4., -3., 4., 4., 1.))
ODD_GRID = ((1, 5, 7), (-4., -4., -3., 4., 4., 1.))                   # 35 cells: no power of two, one digit pass
WIDE_GRID = ((1, 64, 64), (-4., -4., -3., 4., 4., 1.))                # 4096 cells + the sentinel: 13 bits, a second 8-bit digit pass
WIDE_W = 64


def crowd_sensor(grid, pc_range, mode, width, normalize=True):
    return FiveSteep(width=width, grid_sizes=list(grid), pc_range=list(pc_range), normalize_volume_densities=normalize, **BU.mode_kw(mode))


@functools.lru_cache(maxsize=None)
def crowded_input(mode, width=CROWD_W):
    """(3, 2, width, 5) fp32, read-only.  Image 0: every pixel between 0.05 and 3 m, so each lies inside the 8 m x 8 m volumes above and
    those under 1.3 m vote into the four centre cells of the 4 x 4 grid whatever their azimuth; image 1: another draw; image 2: image 0
    with every second pixel moved far outside (3 km)."""
    rng = np.random.default_rng(1234)
    shape = (2, width, 5)
    metres = rng.uniform(0.05, 3.0, shape)
    rem = rng.uniform(0, 1, (2, width, 5)).astype(F)
    img = np.empty((CROWD_B, 2, width, 5), F)
    img[:2, 0], img[:2, 1] = BU.encode(metres, mode), rem
    img[2] = img[0]
    far = np.zeros((width, 5), bool)
    far.reshape(-1)[1::2] = True
    img[2, 0][far] = BU.encode(3000.0, mode)
    img.setflags(write=False)
    return img


def flat_votes(t, img, points=None):
    """Per image, in vote order v = n * 8 + (dx * 4 + dy * 2 + dz): (cell, counted, w, w f) as numpy arrays (B, 8 N), from the host's own
    geometry (fp32, the library's tables; points: the device's, if given)."""
    x = torch.from_numpy(np.array(img, F))
    B = x.shape[0]
    pts = None if points is None else torch.from_numpy(np.array(points, F))
    geo = t._bev_geometry(x, pts, tables="library")
    cols = [[], [], [], []]
    for _, _, _, idx, ok, wx, wy, wz in t._bev_votes(geo):
        w = (wx * wy) * wz
        for col, v in zip(cols, (idx, ok & (w != 0), w, w * geo["f"])):
            col.append(v.reshape(B, -1))
    return tuple(torch.stack(c, 2).reshape(B, -1).numpy() for c in cols)


def loop_sums(votes, nvox, descending=False):
    """The contract, literally: every counted vote, in ascending (or descending) v, is added to its cell with one fp32 addition."""
    cell, counted, w, wf = votes
    B, M = cell.shape
    d, S = np.zeros((B, nvox), F), np.zeros((B, nvox), F)
    order = range(M - 1, -1, -1) if descending else range(M)
    for b in range(B):
        cb, kb, wb, fb, db, Sb = cell[b], counted[b], w[b], wf[b], d[b], S[b]
        for v in order:
            if kb[v]:
                c = cb[v]
                db[c] = F(db[c] + wb[v])
                Sb[c] = F(Sb[c] + fb[v])
    return d, S


def order_sensitive_cells(votes, nvox):
    up, down = loop_sums(votes, nvox), loop_sums(votes, nvox, descending=True)
    return (bits(up[0]) != bits(down[0])) | (bits(up[1]) != bits(down[1])), up


# ---- the statement -----------------------------------------------------------------------------------------------------------------------
@GRID_CASES
@MODE_CASES
def test_host_statement_is_the_literal_loop_and_within_the_bounds(grid, pc_range, mode):
    t = BU.bev_sensor(grid, pc_range, mode)
    o = BU.oracle_of(t)
    img = np.array(BU.bev_input(grid, pc_range, mode)[0])
    gz = grid[0]
    nvox = int(np.prod(grid))
    pc = o.to_pc(img)
    vox, d, S = t.to_voxel_ordered_host(img, points=pc)
    assert vox.dtype == d.dtype == S.dtype == F and vox.shape == (BU.SPLAT_B, 2 * gz) + tuple(grid[1:]) and d.shape == (BU.SPLAT_B,) + tuple(grid)
    ld, lS = loop_sums(flat_votes(t, img, pc), nvox)
    assert np.array_equal(bits(d.reshape(BU.SPLAT_B, -1)), bits(ld)) and np.array_equal(bits(S.reshape(BU.SPLAT_B, -1)), bits(lS))
    assert np.array_equal(bits(t.to_voxel_ordered_host(torch.from_numpy(img), points=torch.from_numpy(pc), return_raw=False)), bits(vox))
    # without points the geometry is the host's own: the same function of the image
    _, d2, _ = t.to_voxel_ordered_host(img)
    assert np.array_equal(bits(d2.reshape(BU.SPLAT_B, -1)), bits(loop_sums(flat_votes(t, img), nvox)[0]))
    # within the bound a k-term fp32 sum has in ANY order, against the fp64 accumulation of the same votes
    ref = BU.splat_reference(o, pc)
    _, bound_d, bound_f = BU.splat_bounds(ref)
    want = o.to_voxel(img, pc=pc).astype(np.float64)
    occ = ref["k"] > 0
    assert np.array_equal(d != 0, occ) and (bits(d)[~occ] == 0).all() and (bits(S)[~occ] == 0).all()          # +0.f, not -0.f
    assert (np.abs(d.astype(np.float64) - ref["sw"]) <= bound_d).all()
    assert (np.abs(vox[:, :gz].astype(np.float64) - want[:, :gz]) <= bound_d + 2e-5).all()
    assert (np.abs(vox[:, gz:].astype(np.float64) - want[:, gz:]) <= bound_f).all()


def test_host_statement_refuses_what_it_cannot_read():
    t = BU.bev_sensor(*BU.SPLAT_GRIDS[0], "linear")
    with pytest.raises(ValueError):
        t.to_voxel_ordered_host(np.zeros((1, 2, 37, 4), F))
    with pytest.raises(ValueError):
        t.to_voxel_ordered_host(np.zeros((1, 1, 37, 5), F))
    vox, d, S = t.to_voxel_ordered_host(np.full((1, 2, 37, 5), BU.encode(3000.0, "linear"), F))                # nothing inside: all +0
    assert not bits(vox).any() and not bits(d).any() and not bits(S).any()


# ---- the inputs can tell orders apart -----------------------------------------------------------------------------------------------------
@GRID_CASES
@MODE_CASES
def test_bev_input_tells_ascending_from_descending(grid, pc_range, mode):
    """A device that summed a cell's votes in another order could not pass the bit-exact tests by luck: in at least 10 cells of every
    case the descending sum has other bits.  The cells hold up to 27 votes: both sides of ORD_SHORT."""
    t = BU.bev_sensor(grid, pc_range, mode)
    img = np.array(BU.bev_input(grid, pc_range, mode)[0])
    votes = flat_votes(t, img)
    nvox = int(np.prod(grid))
    differ, _ = order_sensitive_cells(votes, nvox)
    assert differ.sum() >= 10, int(differ.sum())
    per_cell = np.stack([np.bincount(votes[0][b][votes[1][b]], minlength=nvox) for b in range(BU.SPLAT_B)])
    assert per_cell.max() > ORD_SHORT and ((per_cell > 0) & (per_cell <= ORD_SHORT)).any()


@MODE_CASES
@pytest.mark.parametrize("grid,pc_range,width", [CROWD_GRID + (CROWD_W,), ODD_GRID + (CROWD_W,), WIDE_GRID + (WIDE_W,)],
                         ids=["1x4x4", "1x5x7", "1x64x64"])
def test_crowded_input_is_what_the_gpu_tests_need(grid, pc_range, width, mode):
    t = crowd_sensor(grid, pc_range, mode, width)
    img = np.array(crowded_input(mode, width))
    votes = flat_votes(t, img)
    cell, counted, _, _ = votes
    nvox = int(np.prod(grid))
    M = cell.shape[1]
    assert M == 8 * width * 5
    differ, (d, _) = order_sensitive_cells(votes, nvox)
    occupied = d != 0
    if grid == WIDE_GRID[0]:                       # sparse on purpose: the case is about the second digit pass, cells above 255 in use
        assert nvox + 1 > 2 ** 8 and (cell[counted] > 255).any() and occupied.sum() > 256
        return
    assert differ.sum() >= 0.5 * occupied.sum(), (int(differ.sum()), int(occupied.sum()))
    nchunks = -(-M // ORD_CHUNK)
    assert nchunks >= 3 and M % ORD_CHUNK != 0 and M % ORD_ROUND != 0
    per_cell = np.stack([np.bincount(cell[b][counted[b]], minlength=nvox) for b in range(CROWD_B)])
    if grid == CROWD_GRID[0]:
        # 2545 pixels cast at most 4 counted votes each (one z plane: the dz = 1 corner is outside), about 10 000 a image over 16
        # cells: the four centre cells take over 1000 each (more than 16 wave loads of 64), every other cell more than ORD_SHORT
        assert (per_cell[0] > 1000).sum() >= 4 and (per_cell > ORD_SHORT).all(), per_cell[0]
    for b in range(CROWD_B):                       # a cell that takes votes from every chunk of the image
        chunk_of = np.arange(M) // ORD_CHUNK
        best = int(np.argmax(per_cell[b]))
        assert len(np.unique(chunk_of[counted[b] & (cell[b] == best)])) == nchunks
    assert (img[2, 0].reshape(-1)[1::2] == BU.encode(3000.0, mode)).all() and np.array_equal(img[2, 0].reshape(-1)[::2], img[0, 0].reshape(-1)[::2])
    assert not np.array_equal(img[0], img[1])


# ---- wiring that needs no GPU -----------------------------------------------------------------------------------------------------------
def _args(*extra):
    return CLI.build_parser().parse_args(["--out", "o", "--steps", "1", *extra])


def test_command_line_takes_bev_ordered():
    assert _args().bev_ordered is False
    bev = ("--discriminator", "patchgan", "--disc-bev", "--bev-rec-weight", "1")
    CLI.check_args(_args(*bev, "--deterministic", "--bev-ordered"))
    CLI.check_args(_args(*bev, "--bev-ordered"))                                        # an ordered splat in an unordered step
    CLI.check_args(_args("--bev-ordered"))                                              # no BEV term: accepted, never read
    for old in ((*bev, "--deterministic"), ("--bev-rec-weight", "1", "--deterministic")):
        with pytest.raises(ValueError, match="--bev-ordered"):
            CLI.check_args(_args(*old))


def test_keywords_exist_with_their_defaults():
    import inspect

    from rangeldm_amd import range_image as RI
    from rangeldm_amd.vae_training import VAEDecoderTrainer, VAETrainer
    for fn in (RI.point_cloud_to_range_image.to_voxel, RI.point_cloud_to_range_image.to_voxel_train):
        assert inspect.signature(fn).parameters["ordered"].default is False
    for cls in (VAEDecoderTrainer, VAETrainer):
        assert inspect.signature(cls.__init__).parameters["bev_ordered"].default is False
    p = inspect.signature(RI.point_cloud_to_range_image.to_voxel_ordered_host).parameters
    assert p["points"].default is None and p["tables"].default == "library" and p["return_raw"].default is True
