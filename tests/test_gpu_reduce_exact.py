"""Column sums, the scalar sum and segment pooling on integer-valued data.

Inputs are random integers in [-8, 8] stored as fp32 (or bf16): every partial
sum is an integer below 2^24 in magnitude, so ANY summation order is exact and
the kernels are held to torch.equal against an integer reference.  A lost,
doubled or shifted row cannot hide in a norm.  The shapes are the smallest
that reach each edge of the partition plan (make_band / band_parts, mirrored
below and asserted, so a change of the plan fails here instead of silently
moving the cases off the edges)."""
import pytest
import torch

from molclr_amd import _lib

from .rounding import rne_bf16

gpu = pytest.mark.gpu

GUARD = 4096


# --- the host-side plan (csrc/common.h make_band, csrc/norm.hip band_parts) ---
def make_band(dim):
    d4 = dim // 4
    band = max(256 // d4, 1)
    if band * d4 < 192 and (band + 1) * d4 <= 1024:
        band += 1
    while band * d4 > 1024:
        band -= 1
    return d4, band, (band * d4 + 63) // 64 * 64


def band_parts(rows, band):
    return min(max(-(-rows // (band * 16)), 1), 1024)


def test_plan_mirror_matches_the_issue_table():
    assert make_band(4)[1] == 256
    assert make_band(300) == (75, 3, 256)     # 225 live lanes of 256
    assert make_band(600) == (150, 2, 320)    # 300 live of 320
    assert make_band(1028)[:2] == (257, 1)
    assert make_band(4096) == (1024, 1, 1024)


def ints(shape, dev, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(dtype).to(dev)


def colsum(lib, dev, xptr, out, rows, cols, ld, acc):
    wsb = lib.molclr_colsum_f32_workspace_bytes(rows, cols)
    assert wsb == band_parts(rows, make_band(cols)[1]) * cols * 4 + 256
    ws = torch.full((wsb + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    rc = lib.molclr_colsum_f32(xptr, out.data_ptr(), rows, cols, ld, acc, ws.data_ptr(), wsb, None)
    assert rc == 0, lib.molclr_last_error()
    torch.cuda.synchronize()
    assert (ws[wsb:] == 0x5A).all(), "molclr_colsum_f32 wrote past its workspace"


def colsum_rows(D):
    band = make_band(D)[1]
    rows = {0, 1, band - 1, band * 16, band * 16 + 1}
    if band == 1:
        rows |= {2, 15}   # band - 1 == 0 is there already: a partition's ragged end
    return sorted(rows)


COLSUM_CASES = [(D, r) for D in (4, 300, 600, 1028, 4096) for r in colsum_rows(D)]
# the cap at 1024 partitions; there rows_per_part * 1023 >= rows, so trailing
# partitions are empty (below the cap rows_per_part <= 16 band, and the last
# partition always has a row: the cap is the only way to an empty one)
COLSUM_CASES += [(600, 33000), (1028, 16500)]


@gpu
@pytest.mark.parametrize("D,rows", COLSUM_CASES)
def test_colsum_exact(dev, D, rows):
    lib = _lib.load()
    band = make_band(D)[1]
    P = band_parts(rows, band)
    if rows > 10000:
        rpp = -(-rows // P)
        assert P == 1024 and rows > 1024 * band * 16 and rpp * (P - 1) >= rows
    x = ints((max(rows, 1), D), dev, 1000 * D + rows)[:rows]
    ref = x.double().sum(0)
    assert 8 * rows < 2 ** 24   # no partial sum can round
    out = torch.full((D,), float("nan"), device=dev)
    colsum(lib, dev, x.data_ptr(), out, rows, D, D, 0)
    assert torch.equal(out.double(), ref)
    # accumulate onto a non-zero integer out; rows == 0 leaves it unchanged
    base = ints((D,), dev, 7 + D) * 3 + 1
    out = base.clone()
    colsum(lib, dev, x.data_ptr(), out, rows, D, D, 1)
    assert torch.equal(out.double(), base.double() + ref)
    if rows == 0:
        assert torch.equal(out, base)


@gpu
@pytest.mark.parametrize("D,rows", [(300, 49), (600, 33), (4, 300), (1028, 17)])
def test_colsum_leading_dimension(dev, D, rows):
    """X is a view into a wider matrix whose other columns are NaN: one read
    outside the view's columns poisons a sum."""
    lib = _lib.load()
    ld = D + 8
    wide = torch.full((rows, ld), float("nan"), device=dev)
    wide[:, 4:4 + D] = ints((rows, D), dev, D + rows)
    out = torch.full((D,), float("nan"), device=dev)
    colsum(lib, dev, wide.data_ptr() + 16, out, rows, D, ld, 0)
    assert torch.equal(out.double(), wide[:, 4:4 + D].double().sum(0))


@gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_sum_exact(dev, n):
    lib = _lib.load()
    x = ints((max(n, 1),), dev, n)[:n]
    out = torch.full((1,), float("nan"), device=dev)
    assert lib.molclr_sum_f32(x.data_ptr() if n else None, out.data_ptr(), n, None) == 0
    torch.cuda.synchronize()
    assert out.double().item() == x.double().sum().item()


# --- segment pooling --------------------------------------------------------
SEG_LEN = [0, 1, 7, 8, 9, 15, 16, 17, 40, 0]   # around the 8-row unroll and its tail
PAD_LO, PAD_HI = 3, 5                          # rows before ptr[0] and after ptr[G]


def pool_case(dev):
    G = len(SEG_LEN)
    ptr = [PAD_LO]
    for n in SEG_LEN:
        ptr.append(ptr[-1] + n)
    N = ptr[-1] + PAD_HI
    assert ptr[0] == 3 and ptr[G] == N - 5
    return G, N, ptr, torch.tensor(ptr, dtype=torch.int32, device=dev)


@gpu
@pytest.mark.parametrize("mode", ["mean", "add"])
@pytest.mark.parametrize("D", [4, 300, 512])   # G * D/4 = 10, 750, 1280 threads: blocks of 256
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_segment_pool_exact(dev, dtype, D, mode):
    lib = _lib.load()
    G, N, ptr, dptr = pool_case(dev)
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    sfx = "_bf16" if dtype == "bf16" else ""
    m = 0 if mode == "mean" else 1
    h = ints((N, D), dev, D + m, tdt)
    h[:PAD_LO] = float("nan")          # padding rows belong to no graph: never read
    h[N - PAD_HI:] = float("nan")
    cnt = torch.tensor(SEG_LEN, dtype=torch.float64, device=dev).clamp_min(1).unsqueeze(1)
    seg_sum = torch.stack([h[ptr[g]:ptr[g + 1]].double().sum(0) for g in range(G)])
    # mean: an exact sum, then ONE correctly rounded fp32 division (no fast-math
    # in the build; the fp64 quotient rounded to fp32 is that division's result:
    # 53 >= 2 * 24 + 2 bits make the double rounding innocuous)
    ref = seg_sum if mode == "add" else (seg_sum / cnt).float().double()
    out = torch.full((G, D), float("nan"), device=dev)
    rc = getattr(lib, "molclr_segment_pool_fwd" + sfx)(h.data_ptr(), dptr.data_ptr(),
                                                       out.data_ptr(), G, D, m, None)
    assert rc == 0, lib.molclr_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.double(), ref)

    # backward: every row of graph g gets dout[g] (add) or dout[g] / cnt, one
    # fp32 rounding (then one round-to-nearest-even to bf16 storage); padding
    # rows get exactly 0 -- dh starts as NaN
    g_ = torch.Generator().manual_seed(D)
    dout = torch.randn(G, D, generator=g_).to(dev)
    dh = torch.full((N, D), float("nan"), dtype=tdt, device=dev)
    rc = getattr(lib, "molclr_segment_pool_bwd" + sfx)(dout.data_ptr(), dptr.data_ptr(),
                                                       dh.data_ptr(), N, G, D, m, None)
    assert rc == 0, lib.molclr_last_error()
    torch.cuda.synchronize()
    val = dout.double() if mode == "add" else (dout.double() / cnt).float().double()
    if dtype == "bf16":
        val = rne_bf16(val.cpu()).to(dev)
    exp = torch.zeros(N, D, dtype=torch.float64, device=dev)
    for g in range(G):
        exp[ptr[g]:ptr[g + 1]] = val[g]
    assert torch.equal(dh.double(), exp)
