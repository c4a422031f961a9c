"""Helpers of the exact single-layer tests: inputs for which every product and every partial sum is exact in fp32, so that a HIP
result must equal a float64 restatement bit for bit in any summation order.

* the integer layers and the launcher wrapper of tests/test_half_exact.py (16-bit storage) and tests/test_f32_exact.py;
* the shape rules of the fp32 direct variants, the Winograd forms and nd_layer_wgrad, each derived from the launch code, with the
  Python mirrors of that launch code the rules rest on (tests/test_f32_exact_host.py checks the mirrors and the rules on the CPU);
* float64 / fp32 restatements of the Winograd algorithm and the L1 bounds that decide whether a case is order-free exact.
"""
import math
import re

import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib

KBLOCKS = {"f32": 8, "bf16": 16, "f16": 16}      # input channels per K block
NAME = re.compile(r"^(f32|bf16|f16)_m(\d+)x(\d+)_n(\d+)x(\d+)_t(\d+)_k(\d+)_up(true|false)_s(\d+)$")


def variants(dtype):
    """Every conv_qp variant of one storage type, in index order: its ABI index, name and workgroup shape."""
    lib = _lib.load()
    out = []
    for v in range(lib.nd_num_conv_variants()):
        m = NAME.match(lib.nd_conv_variant_name(v).decode())
        if m and m.group(1) == dtype:
            mr, wm, nr, wn, taps, kbc = (int(m.group(i)) for i in range(2, 8))
            out.append(dict(v=v, name=m.group(0), mblk=32 * mr * wm, nblk=32 * nr * wn, taps=taps, kbc=kbc, up=m.group(8) == "true"))
    return out


def _mismatch(got, want):
    return f"{int((got != want).sum())} of {want.numel()} values differ (NaN: {int(torch.isnan(got).sum())})"


def _grid_of(count, min_rows):
    """(rows, cols) with rows * cols == count, both >= min_rows, cols no multiple of 8, as square as possible; None if there is none."""
    best = None
    for rows in range(min_rows, count // min_rows + 1):
        cols = count // rows
        if count % rows == 0 and cols % 8 and (best is None or abs(rows - cols) < abs(best[0] - best[1])):
            best = (rows, cols)
    return best


def _pixel_grids(nblk, kind):
    """Valid grids of nblk - 1 and nblk + 1 pixels per image.  A 3x3 transposed layer has at least three output rows; where
    nblk + 1 has no such factorisation (257 is prime) it takes the next count above that has one."""
    min_rows = 3 if kind == "convT3" else 1
    grids = []
    for count in (nblk - 1, nblk + 1):
        while _grid_of(count, min_rows) is None:
            assert kind == "convT3" and count > nblk
            count += 1
        grids.append(_grid_of(count, min_rows))
    return grids


def _integer_layer(kind, cin, cout, h, w, seed, batch=3):
    """Dense small integers (|x| <= 3, |w| <= 2, integer bias): the largest sum, 3 * 2 * 9 * cin + 8, is below 2^14 for cin <= 320
    and below 2^24 for every cin a test uses: exact."""
    g = torch.Generator().manual_seed(seed)
    k = {"conv3": 3, "convT3": 3, "conv1": 1, "conv2s2": 2, "convT2s2": 2}[kind]
    x = torch.randint(-3, 4, (batch, cin, h, w), generator=g).float()
    wt = torch.randint(-2, 3, (cout, cin, k, k) if kind in ("conv3", "conv1", "conv2s2") else (cin, cout, k, k), generator=g).float()
    b = torch.randint(-8, 9, (cout,), generator=g).float()
    return x, wt, b


def _linear_layer(kind, x, w, b):
    if kind in ("conv3", "conv1"):
        return F.conv2d(x, w, b)
    if kind == "conv2s2":
        return F.conv2d(x, w, b, stride=2)
    return F.conv_transpose2d(x, w, b, stride=2 if kind == "convT2s2" else 1)


def _expected_layer(kind, x, w, b, act, slope, tdt):
    x, w, b = x.double(), w.double(), b.double()
    y = _linear_layer(kind, x, w, b)
    if act == "PReLU":
        y = torch.where(y > 0, y, y * slope)
    return y.to(tdt).float()


def _layer_forward(dev, kind, x, w, b, act, slope, variant, dtype, flags):
    """nd_layer_forward into a NaN-prefilled output (layer_forward of test_hip_parity.py), or None where the launcher refuses the
    pair of variant and shape with ND_EINVAL."""
    lib = _lib.load()
    k, dt = _lib.KIND[kind], _lib.DTYPE[dtype]
    B, cin, H, W = x.shape
    cout = w.shape[0] if kind in ("conv3", "conv1", "conv2s2") else w.shape[1]
    nbytes = lib.nd_layer_packed_bytes(k, cin, cout, dt)
    packed = torch.empty(nbytes // 4, dtype=torch.float32)
    wc, bc = w.contiguous(), b.contiguous()
    _lib.check(lib.nd_layer_pack(k, cin, cout, dt, wc.data_ptr(), bc.data_ptr(), packed.data_ptr(), nbytes))
    packed = packed.to(dev)
    oh, ow = {"conv3": (H - 2, W - 2), "convT3": (H + 2, W + 2), "convT2s2": (2 * H, 2 * W), "conv1": (H, W),
              "conv2s2": (H // 2, W // 2)}[kind]
    y = torch.full((B, cout, oh, ow), float("nan"), dtype=torch.float32, device=dev)
    wsb = lib.nd_layer_workspace_bytes(k, B, cin, cout, H, W, dt)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    xd = x.to(dev).contiguous()
    rc = lib.nd_layer_forward(k, _lib.ACT[act], slope, dt, packed.data_ptr(), xd.data_ptr(), B, cin, H, W, cout, y.data_ptr(),
                              ws.data_ptr(), wsb, variant, flags, _lib.stream_ptr(dev))
    if rc == -1:        # ND_EINVAL
        return None
    _lib.check(rc, "nd_layer_forward")
    torch.cuda.synchronize()
    return y.cpu()


def log2_of(bound):
    return math.log2(max(float(bound), 1.0))


# ---------------------------------------------------------------------------- 1. the fp32 direct variants

BATCH = 3       # tiles cross image seams where the launcher lets them
SLOPE = 0.5


def f32_variant_shapes(V):
    """(kind, cin, cout, H, W) of every case of one fp32 variant, by the rules of test_half_exact._variant_shapes with the fp32 units:
    a plane holds 4 channels (the only step the launcher demands of cout) and a K block 8.

    * nblk - 1 and nblk + 1 valid pixels per image at a row width that is no multiple of 8 (_pixel_grids);
    * cout one plane below and above mblk (a 2x2 stride-2 transpose has M = 4 * cout rows: below and above mblk / 4);
    * K blocks {1, 4 * kbc + 1, kbc, 5 * kbc}: one block, a remainder against the variant's K chunk (refused for kbc > 1), one
      chunk, five chunks;
    * the 9-tap variants also at cin = 3: the first layer, three channels padded into one K block."""
    kinds = {9: ("conv3", "convT3"), 1: ("conv1",), 4: ("conv2s2",)}[V["taps"]] if not V["up"] else ("convT2s2",)
    couts = (V["mblk"] // 4 - 4, V["mblk"] // 4 + 4) if V["up"] else (V["mblk"] - 4, V["mblk"] + 4)
    cins = [kb * KBLOCKS["f32"] for kb in sorted({1, 4 * V["kbc"] + 1, V["kbc"], 5 * V["kbc"]})]
    if V["taps"] == 9:
        cins = [3] + cins
    cases = []
    for kind in kinds:
        for hv, wv in _pixel_grids(V["nblk"], kind):
            h, w = {"conv3": (hv + 2, wv + 2), "convT3": (hv - 2, wv - 2), "conv1": (hv, wv), "conv2s2": (2 * hv, 2 * wv),
                    "convT2s2": (hv, wv)}[kind]
            cases += [(kind, cin, cout, h, w) for cin in cins for cout in couts]
    return cases


def valid_pixels(kind, h, w):
    """Pixels per image that an N tile of conv_qp enumerates (valid_grid of conv_f32.hip): the outputs, or for the 2x2 stride-2
    transpose the inputs."""
    return {"conv3": (h - 2) * (w - 2), "convT3": (h + 2) * (w + 2), "conv1": h * w, "conv2s2": (h // 2) * (w // 2),
            "convT2s2": h * w}[kind]


def dropped_part_changes(kind, x, w, what):
    """Does the float64 layer change when the last valid pixel of the last image ('pixel') or the last input channel ('channel') is
    dropped?  The layer is linear before its activation and PReLU with a non-zero slope is one-to-one, so the result changes
    exactly where the dropped part's own contribution is not zero."""
    part = torch.zeros_like(x[-1:])
    if what == "pixel":
        part[:, :, -1, -1] = x[-1, :, -1, -1]
    else:
        part[:, -1] = x[-1, -1]
    return bool(_linear_layer(kind, part.double(), w.double(), None).ne(0).any())


def direct_l1(kind, x, w, b):
    """Largest sum of magnitudes behind one output: every partial sum in any order stays below it."""
    return float((_linear_layer(kind, x.double().abs(), w.double().abs(), b.double().abs())).max())


# ---------------------------------------------------------------------------- 2. the Winograd forms

# tile code -> (T, three-pass 2-D form?, weight multiplier that makes G g (G^T) integer).  F(6x6) has none: 1/32 next to 32 in A^T
# and 5.25 / 4.25 in B^T need more than 24 bits on any dense data
WINO_FORMS = {1: (2, False, 2), 2: (2, True, 4), 3: (4, False, 24), 4: (4, True, 576), 5: (4, False, 24), 6: (6, True, 1)}
WINO_CODE4_EXACT_CIN = 64       # F(4x4) with +-1 data: log2(L1) ~ 22.9 at 64 channels, ~ 23.8 at 128

_M = {
    2: dict(BT=[[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
            GD=[[2, 0, 0], [1, 1, 1], [1, -1, 1], [0, 0, 2]], D=2,
            AT=[[1, 1, 1, 0], [0, 1, -1, -1]]),
    4: dict(BT=[[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                [0, 4, 0, -5, 0, 1]],
            GD=[[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], D=24,
            AT=[[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]),
    6: dict(BT=[[1, 0, -5.25, 0, 5.25, 0, -1, 0], [0, 1, 1, -4.25, -4.25, 1, 1, 0], [0, -1, 1, 4.25, -4.25, -1, 1, 0],
                [0, .5, .25, -2.5, -1.25, 2, 1, 0], [0, -.5, .25, 2.5, -1.25, -2, 1, 0], [0, 2, 4, -2.5, -5, .5, 1, 0],
                [0, -2, 4, 2.5, -5, -.5, 1, 0], [0, -1, 0, 5.25, 0, -5.25, 0, 1]],
            GD=[[90, 0, 0], [-20, -20, -20], [-20, 20, -20], [1, 2, 4], [1, -2, 4], [64, 32, 16], [64, -32, 16], [0, 0, 90]], D=90,
            AT=[[1, 1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, .5, -.5, 0], [0, 1, 1, 4, 4, .25, .25, 0], [0, 1, -1, 8, -8, .125, -.125, 0],
                [0, 1, 1, 16, 16, .0625, .0625, 0], [0, 1, -1, 32, -32, .03125, -.03125, 1]]),
}


def wino_matrices(T):
    """B^T, D * G, A^T of F(T,3) as winograd.hip (Wino<T>) and conv_w1d.hip (W1<T>) state them, in float64, and D: G is kept as the
    integer matrix D * G, so that (D G) g (D G)^T / D^2 rounds once -- and not at all where the weights are multiples of D (D^2)."""
    return tuple(torch.tensor(_M[T][k], dtype=torch.float64) for k in ("BT", "GD", "AT")) + (_M[T]["D"],)


def wino_group(code, cin):
    """'exact': the GPU must equal float64 bit for bit; 'f64': held to 10 x the error of the fp32 restatement."""
    return "exact" if code in (1, 2, 3, 5) or (code == 4 and cin <= WINO_CODE4_EXACT_CIN) else "f64"


def wino_layer(code, kind, cin, cout, h, w, seed, batch=BATCH):
    """Integer x and bias, weights = the code's multiplier x small integers.  |x| <= 3 and |w / m| <= 2, for F(4x4) |x| <= 1 and
    |w / 576| <= 1 (its transforms gain ~ 100 x 100)."""
    mult = WINO_FORMS[code][2]
    xmax, kmax = (1, 1) if code == 4 else (3, 2)
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-xmax, xmax + 1, (batch, cin, h, w), generator=g).float()
    wt = torch.randint(-kmax, kmax + 1, (cout, cin, 3, 3) if kind == "conv3" else (cin, cout, 3, 3), generator=g).float() * mult
    b = torch.randint(-8, 9, (cout,), generator=g).float()
    return x, wt, b


def wino_restate(code, kind, x, w, b, slope, dt=torch.float64, bound=False):
    """The Winograd algorithm of one tile code, restated with torch on the CPU: the weights transformed in double and cast to dt,
    B^T d (B), one matrix product per position summed over the input channels (and over the three kernel rows in the 1-D forms),
    A^T m (A), bias, PReLU -- everything after the weight transform in dt.

    bound=True: the L1 bound instead, max over the outputs of sum |U| |V| pushed through |A^T| (|A|), plus |bias|: below 2^24, every
    partial sum of every summation order is an integer that fp32 holds (with integer U and V)."""
    T, two_d, _ = WINO_FORMS[code]
    BT, G, AT, D = wino_matrices(T)
    A = T + 2
    x, w = x.double(), w.double()
    if kind == "convT3":        # the same valid correlation on the zero-bordered input with flipped, transposed weights
        x = F.pad(x, (2, 2, 2, 2))
        w = w.flip(2, 3).transpose(0, 1)
    Hv, Wv = x.shape[2] - 2, x.shape[3] - 2
    ty, tx = (Hv + T - 1) // T, (Wv + T - 1) // T
    if two_d:
        U = torch.einsum("ak,oikl,bl->oiab", G, w, G) / (D * D)
        d = F.pad(x, (0, T * tx - Wv, 0, T * ty - Hv)).unfold(2, A, T).unfold(3, A, T)       # [B, cin, ty, tx, A, A]
    else:
        U = torch.einsum("ak,oiyk->oiya", G, w) / D                                           # [cout, cin, ky, A]
        d = F.pad(x, (0, T * tx - Wv)).unfold(3, A, T)                                        # [B, cin, Hb, tx, A]
    if bound:
        V = (torch.einsum("ai,ncyxij,bj->ncyxab", BT, d, BT) if two_d else torch.einsum("aj,nchgj->nchga", BT, d)).abs()
        U, AT = U.abs(), AT.abs()
        bias = b.double().abs()
    else:
        U, d, BT, AT, bias = U.to(dt), d.to(dt), BT.to(dt), AT.to(dt), b.to(dt)
        V = torch.einsum("ai,ncyxij,bj->ncyxab", BT, d, BT) if two_d else torch.einsum("aj,nchgj->nchga", BT, d)
    if two_d:
        M = torch.einsum("oiab,niyxab->noyxab", U, V)
        y = torch.einsum("ta,noyxab,ub->noytxu", AT, M, AT).reshape(x.shape[0], U.shape[0], T * ty, T * tx)[:, :, :Hv, :Wv]
    else:
        M = sum(torch.einsum("oia,nihga->nohga", U[:, :, ky], V[:, :, ky:ky + Hv]) for ky in range(3))
        y = torch.einsum("ta,nohga->nohgt", AT, M).reshape(x.shape[0], U.shape[0], Hv, T * tx)[:, :, :, :Wv]
    y = y + bias.view(1, -1, 1, 1)
    if bound:
        return float(y.max())
    return torch.where(y > 0, y, y * slope)


def wino_packed(code, kind, cin, cout, w, b):
    """nd_winograd_pack on the host: the blob as fp32 values."""
    lib = _lib.load()
    nbytes = lib.nd_winograd_packed_bytes(code, cin, cout)
    packed = torch.empty(nbytes // 4, dtype=torch.float32)
    wc, bc = w.contiguous(), b.contiguous()
    _lib.check(lib.nd_winograd_pack(code, _lib.KIND[kind], cin, cout, wc.data_ptr(), bc.data_ptr(), packed.data_ptr(), nbytes),
               "nd_winograd_pack")
    return packed


def wino_forward(dev, code, kind, x, w, b, act, slope, flags):
    """nd_layer_forward_winograd into a NaN-prefilled output, or None where the launcher refuses the shape with ND_EINVAL."""
    lib = _lib.load()
    B, cin, H, W = x.shape
    cout = w.shape[0] if kind == "conv3" else w.shape[1]
    packed = wino_packed(code, kind, cin, cout, w, b).to(dev)
    oh, ow = (H - 2, W - 2) if kind == "conv3" else (H + 2, W + 2)
    y = torch.full((B, cout, oh, ow), float("nan"), dtype=torch.float32, device=dev)
    wsb = lib.nd_layer_winograd_workspace_bytes(code, _lib.KIND[kind], B, cin, cout, H, W)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    xd = x.to(dev).contiguous()
    rc = lib.nd_layer_forward_winograd(code, _lib.KIND[kind], _lib.ACT[act], slope, packed.data_ptr(), xd.data_ptr(), B, cin, H, W, cout,
                                       y.data_ptr(), ws.data_ptr(), wsb, flags, _lib.stream_ptr(dev))
    if rc == -1:        # ND_EINVAL
        return None
    _lib.check(rc, "nd_layer_forward_winograd")
    torch.cuda.synchronize()
    return y.cpu()


def gemm_variant(cin, cout):
    """Mirror of nd_conv_variant_gemm (conv_f32.hip) followed by pick_variant's 1-tap choice where that returns -1: the index, among
    the fp32 variants in ABI order, of the 1-tap GEMM behind a three-pass launch."""
    kb = (cin + 7) // 8
    extra = 15      # the fp32-only variants follow the 15 of the group
    if kb % 2 == 0 and cout % 256 == 0:
        return extra + (4 if kb % 4 == 0 else 2)
    if kb % 2 == 0 and cout % 128 == 0:
        return extra + (5 if kb % 4 == 0 else 3)
    return 5 if kb % 2 else 4


# (cin, cout) for each branch of nd_conv_variant_gemm: KB % 4 != 0 with cout % 256 == 0; KB % 4 == 0 with cout % 256 == 0; KB % 4
# != 0 / == 0 with cout % 128 == 0 only; a cout of 4 k with neither factor and no multiple of 32 (the automatic choice).  The
# KB-odd branch needs cin % 16 != 0, which the three-pass launcher refuses: (24, 36) is that refusal
GEMM_PAIRS = [(16, 256), (32, 256), (16, 128), (32, 128), (16, 36)]
KB_ODD_PAIR = (24, 36)


def _tile_grid(count):
    """(batch, rows, cols) with batch * rows * cols == count: batch 3 where 3 divides count, else 1; rows x cols as square as
    possible (a prime count is one row)."""
    batch = BATCH if count % BATCH == 0 else 1
    n = count // batch
    rows = max(r for r in range(1, math.isqrt(n) + 1) if n % r == 0)
    return batch, rows, n // rows


def _from_output(kind, hv, wv):
    return (hv + 2, wv + 2) if kind == "conv3" else (hv - 2, wv - 2)


class _Kinds:
    """conv3 and convT3 in turn; a transposed layer has at least 3 x 3 outputs."""
    def __init__(self):
        self.n = 0

    def __call__(self, hv, wv):
        self.n += 1
        return "convT3" if self.n % 2 == 0 and min(hv, wv) >= 3 else "conv3"


def wino_tiles(code, batch, kind, h, w):
    """Work items of the launch, mirrored from the launch code: B * TY * TX tiles of T x T outputs (three-pass forms, wino_geo),
    groups of T pixels per image row (1-D forms in conv_w1d), strips of 8 rows x 4 pixels (code 5, conv_w2d)."""
    T = WINO_FORMS[code][0]
    hv, wv = (h - 2, w - 2) if kind == "conv3" else (h + 2, w + 2)
    if WINO_FORMS[code][1]:
        return batch * ((hv + T - 1) // T) * ((wv + T - 1) // T)
    if code == 5:
        return batch * ((hv + 7) // 8) * ((wv + 3) // 4)
    return batch * hv * ((wv + T - 1) // T)


def wino_cases(code):
    """(kind, batch, cin, cout, H, W) of every case of one tile code, by rule; each rule names the launch-code constant it aims at.
    Returns (cases, claims): claims maps a rule to the work-item counts (wino_tiles) or output sizes it promises."""
    T, two_d, _ = WINO_FORMS[code]
    kinds = _Kinds()
    cases, claims = [], {}

    def add(batch, cin, cout, hv, wv, kind=None):
        kind = kind or kinds(hv, wv)
        case = (kind, batch, cin, cout) + _from_output(kind, hv, wv)
        if case not in cases:
            cases.append(case)
        return case

    if two_d:
        # partial tiles in y and x independently: T k - 1, T k, T k + 1 and less than one tile
        sizes = [(2 * T - 1, 3 * T + 1), (3 * T, 2 * T - 1), (2 * T + 1, 3 * T), (T - 1, 2 * T + 1), (3 * T + 1, T - 1)]
        claims["sizes"] = sizes
        for hv, wv in sizes:
            add(BATCH, 16, 20, hv, wv)
        # tile counts one below and above the input-transform block, the output-transform block and the GEMM's nblk; a tile grid
        # of rows x cols has T rows - 1 output rows and one pixel in its last column
        f32 = variants("f32")
        blocks = {"in": (16 if T == 6 else 256, 16, 36), "out": (32 if T == 6 else 128, 16, 36)}
        for cin, cout in GEMM_PAIRS:
            blocks[f"gemm {cin}x{cout}"] = (f32[gemm_variant(cin, cout)]["nblk"], cin, cout)
        for rule, (n, cin, cout) in blocks.items():
            claims[rule] = (n - 1, n + 1)
            for count in (n - 1, n + 1):
                batch, rows, cols = _tile_grid(count)
                add(batch, cin, cout, T * rows - 1, T * (cols - 1) + 1)
        add(BATCH, *KB_ODD_PAIR, 2 * T + 1, 3 * T)
        # deep layers: many channels, few pixels
        for cin in (64, 128, 512):
            add(BATCH, cin, 64, T + 1, 2 * T - 1)
    else:
        # row widths T k - 1, T k, T k + 1 around 64: bordered rows of 65, 66, 67 pixels cross the 64-lane stage pieces (w1d_span)
        sizes = [(7, 63), (9, 64), (8, 65), (3, T - 1), (1, T + 1)]
        claims["sizes"] = sizes
        for hv, wv in sizes:
            add(BATCH, 16, 20, hv, wv)
        # work items per image (batch 3: tiles cross the image seams) / per launch one below and above the workgroup tile
        # (cout one plane below and above the 64-row workgroup tile)
        n = {1: 256, 3: 128, 5: 16}[code]
        claims["tile"] = []
        for count, step in ((n - 1, -1), (n + 1, 1)):
            if code == 5:       # strips are enumerated over the whole batch
                batch, rows, cols = _tile_grid(count)
                hv, wv = 8 * rows - 1, 4 * (cols - 1) + 1
                claims["tile"].append(count)
            else:               # groups per image on at least 3 rows (one row of 257 pairs does not fit the LDS): the nearest count
                while _grid_of(count, 3) is None:       # that factors
                    count += step
                batch, (rows, cols) = BATCH, _grid_of(count, 3)
                hv, wv = rows, T * cols - 1
                claims["tile"].append(BATCH * count)
            for cout in (60, 68):
                add(batch, 16, cout, hv, wv)
        # the first layer (3 channels padded into one K block), an odd number of K blocks, cout of 4 k that is no multiple of 32
        for cin, cout in ((3, 36), (24, 20), (40, 36)):
            add(BATCH, cin, cout, 2 * T + 1, 3 * T - 1)
        add(BATCH, 512, 36, T + 1, 2 * T - 1)
    return cases, claims


# ---------------------------------------------------------------------------- 3. nd_layer_wgrad

def wgrad_geometry(kind, batch, cin, cout, h, w):
    """wg_plan of train.hip: taps, M, N and the common grid gh x gw of the two operands; K = batch * gh * gw."""
    taps = 9 if kind in ("conv3", "convT3") else 1
    if kind in ("conv3", "conv1"):
        gh, gw, m, n = h, w, cout, cin
    elif kind == "convT3":
        gh, gw, m, n = h + 2, w + 2, cin, cout
    else:
        gh, gw, m, n = h, w, cin, cout
    return dict(taps=taps, M=m, N=n, gh=gh, gw=gw, K=batch * gh * gw)


def wgrad_split(taps, m, n, k):
    """Mirror of nd_wgrad_partial_floats (wgrad.hip): K chunks of PC pixels, cut into ksplit slices of cps chunks."""
    pc = 62 if taps == 9 else 64
    mp, np_ = (m + 63) // 64 * 64, (n + 63) // 64 * 64
    chunks = (k + pc - 1) // pc
    tiles = (mp // 64) * (np_ // 64)
    ksplit = max(min(512 // tiles, chunks), 1)
    cps = (chunks + ksplit - 1) // ksplit
    ksplit = (chunks + cps - 1) // cps
    return dict(PC=pc, chunks=chunks, tiles=tiles, cap=512 // tiles, ksplit=ksplit, cps=cps, floats=ksplit * taps * mp * np_,
                last_chunk=k - (chunks - 1) * pc, last_slice=chunks - (ksplit - 1) * cps)


# (kind, batch, cin, cout, H, W): what each case is for stands behind it; test_f32_exact_host.py holds the list to the tables
WGRAD_CASES = [
    ("conv1", 1, 3, 1, 7, 9),           # K = 63 = PC - 1: one short chunk, ksplit 1; M 1, N 3; cout % 4 != 0
    ("conv3", 1, 3, 4, 5, 7),           # K = 35 < PC with 9 taps; M 4, N 3; taps M N = 108
    ("conv3", 1, 64, 63, 6, 31),        # K = 186 = 3 PC: ksplit 3 (the fourth reduce wave has no slice); M 63, N 64
    ("convT3", 1, 65, 4, 3, 35),        # K = 185 = 3 PC - 1: odd last chunk; M 65 (two tiles, rows masked), N 4
    ("conv3", 1, 4, 72, 11, 17),        # K = 187 = 3 PC + 1: one pixel in the last chunk, ksplit 4; M 72, N 4
    ("conv1", 1, 64, 65, 1, 257),       # K = 257 = 4 PC + 1: ksplit 5; H W = 257 for db; a row of 257: three blocks of k_repitch
    ("conv1", 1, 1, 63, 16, 16),        # K = 256 = 4 PC; N 1
    ("conv1", 3, 72, 3, 5, 17),         # K = 255 = 4 PC - 1; M 3, N 72
    ("conv3", 3, 3, 64, 18, 18),        # 16 chunks: ksplit 16 (the unrolled reduce loop alone); M 64
    ("convT3", 3, 4, 3, 15, 18),        # 17 chunks: ksplit 17 (unrolled loop + remainder loop)
    ("convT2s2", 3, 63, 65, 9, 67),     # odd h and w, K = 1809: ksplit 29 with 17 pixels in the last chunk; N 65
    ("conv3", 3, 4, 4, 92, 115),        # 512 chunks on one tile: the cap, 512 slices
    ("conv1", 3, 64, 65, 43, 127),      # K = 16383 = 256 PC - 1 on two tiles: the cap, 256 slices
    ("convT2s2", 3, 65, 72, 19, 143),   # odd h and w, 128 chunks on four tiles: the cap, 128; rows of 143: two blocks of k_repitch
    ("conv3", 3, 4, 3, 84, 129),        # 525 chunks on one tile: cps 2, 263 slices, the last one chunk short; rows of 129
    ("convT3", 3, 65, 65, 48, 51),      # 129 chunks on four tiles: cps 2, 65 slices, the last one chunk short
    ("conv1", 1, 63, 64, 4, 40),        # N 63
    ("conv1", 3, 4, 72, 3, 7),          # K = 63 with batch 3; N 4 ... M 72
]


def wgrad_layer(kind, batch, cin, cout, h, w, seed):
    """Integer x (|x| <= 3) and dy (|dy| <= 2): every sum is an integer below 6 K."""
    g = torch.Generator().manual_seed(seed)
    oh, ow = {"conv3": (h - 2, w - 2), "convT3": (h + 2, w + 2), "convT2s2": (2 * h, 2 * w), "conv1": (h, w)}[kind]
    x = torch.randint(-3, 4, (batch, cin, h, w), generator=g).float()
    dy = torch.randint(-2, 3, (batch, cout, oh, ow), generator=g).float()
    return x, dy


def wgrad_expected(kind, x, dy):
    """float64 autograd of the layer: (dw, db), still float64."""
    k = {"conv3": 3, "convT3": 3, "convT2s2": 2, "conv1": 1}[kind]
    cin, cout = x.shape[1], dy.shape[1]
    w = torch.zeros((cout, cin, k, k) if kind in ("conv3", "conv1") else (cin, cout, k, k), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    _linear_layer(kind, x.double(), w, b).backward(dy.double())
    return w.grad, b.grad


def wgrad_forward(dev, kind, x, dy):
    """nd_layer_wgrad into NaN-prefilled dw and db."""
    lib = _lib.load()
    B, cin, H, W = x.shape
    cout = dy.shape[1]
    k = {"conv3": 3, "convT3": 3, "convT2s2": 2, "conv1": 1}[kind]
    wshape = (cout, cin, k, k) if kind in ("conv3", "conv1") else (cin, cout, k, k)
    wsb = lib.nd_layer_wgrad_workspace_bytes(_lib.KIND[kind], B, cin, cout, H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    dw = torch.full(wshape, float("nan"), device=dev)
    db = torch.full((cout,), float("nan"), device=dev)
    xd, dyd = x.to(dev).contiguous(), dy.to(dev).contiguous()
    _lib.check(lib.nd_layer_wgrad(_lib.KIND[kind], xd.data_ptr(), dyd.data_ptr(), B, cin, H, W, cout, dw.data_ptr(), db.data_ptr(),
                                  ws.data_ptr(), wsb, _lib.stream_ptr(dev)), "nd_layer_wgrad")
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu()
