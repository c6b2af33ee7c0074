"""The conv kernels a full-size training step selects, and one test case per kernel family.

The training path owns no conv kernel: ops._forward calls yolo_conv2d_fwd, and the stride-1 data gradient (yolo_conv2d_bwd_data,
csrc/conv_bwd.hip) is the forward dispatcher run on a transposed pack.  Which kernel runs is decided by the forward's rules from the
map size and the compute-unit count, so a full-size step runs kernels that the small maps of tests/_conv_bwd.py never reach.

    enumerate_step(config)   forward_train on ``meta`` tensors with a recording op table: every conv call of one step as
                             (kind, x shape, weight shape, stride), turned into the descriptors ops._desc and yolo_conv2d_bwd_data build
    family(pick)             a pick string without its `` grid ...`` tail(s): the kernel and its tile
    FAMILY_CASES             (role, family) -> one case; role "forward" (the training forward: act none, bf16 z) or "dgrad" (the
                             stride-1 data gradient).  A case is a tests/_conv_bwd.py case, the stride, and the tuning words it needs.

tests/test_train_families_cpu.py keeps the table complete (every (role, family) of the four configurations has a case that picks it);
tests/test_train_families_gpu.py launches the cases.  The shapes come from tests/diag/family_shape_search.py.
"""
import collections
import re
from types import SimpleNamespace

import torch

import _conv_down as D
import _exact_cases as E

BF16, F32 = torch.bfloat16, torch.float32

# the four full-size configurations: name -> (class, input size, batch, anchors of tests/_cases.py); full width, nc = 80
CONFIGS = {"spp640x8": ("YOLOv3SPP", 640, 8, "SPP_ANCHORS"), "yolov3_416x8": ("YOLOv3", 416, 8, "SPP_ANCHORS"),
           "tiny416x32": ("YOLOv3Tiny", 416, 32, "TINY_ANCHORS"), "lite416x16": ("LiteYOLOv3", 416, 16, "SPP_ANCHORS")}


# ---- the recording op table -------------------------------------------------------------------------------------------------------------
def recording_meta_ops(calls):
    """A table with the signatures of pytorch_yolo_amd.models.train.DEVICE_OPS_POOL on ``meta`` tensors: every function returns a tensor
    of the shape and dtype the device op returns and appends (kind, x shape, weight shape, stride, x requires a gradient) to ``calls``
    for the conv-bearing ops.  The image is the only activation that needs no gradient."""
    def out(x, c, h, w, dtype=BF16):
        return torch.empty((x.shape[0], c, h, w), dtype=dtype, device="meta")

    def rec(kind, x, w, stride):
        calls.append((kind, tuple(x.shape), tuple(w.shape), stride, len(calls) > 0))

    def conv_block(x, w, b=None, *, act="leaky", out_dtype=BF16, stride=1):
        rec("head" if out_dtype == F32 else "conv", x, w, 1)
        return out(x, w.shape[0], x.shape[2], x.shape[3], out_dtype)

    def conv_bn_block(x, w, gamma, beta, rm=None, rv=None, *, training=True, momentum=0.1, eps=1e-5, act="leaky", stride=1):
        rec("bn", x, w, 1)
        return out(x, w.shape[0], x.shape[2], x.shape[3])

    def down_bn_block(x, w, gamma, beta, rm=None, rv=None, *, training=True, momentum=0.1, eps=1e-5, act="leaky"):
        rec("down", x, w, 2)
        return out(x, w.shape[0], *D.out_hw(x.shape[2], x.shape[3]))

    def res_bn_block(x, w, gamma, beta, rm=None, rv=None, residual=None, *, want_preadd=False, training=True, momentum=0.1, eps=1e-5):
        rec("res", x, w, 1)
        y = out(x, w.shape[0], x.shape[2], x.shape[3])
        return (y, torch.empty_like(y)) if want_preadd else y

    def pool_bn_block(x, w, gamma, beta, rm=None, rv=None, *, pool_stride=2, training=True, momentum=0.1, eps=1e-5, act="leaky"):
        rec("poolbn", x, w, 1)
        h, wd = (x.shape[2] // 2, x.shape[3] // 2) if pool_stride == 2 else x.shape[2:]
        return out(x, w.shape[0], h, wd)

    def max_pool(x, *, stride=2):
        h, wd = (x.shape[2] // 2, x.shape[3] // 2) if stride == 2 else x.shape[2:]
        return out(x, x.shape[1], h, wd)

    def spp_concat(x):
        return out(x, 4 * x.shape[1], x.shape[2], x.shape[3])

    def upsample_concat(a, b, *, up_first=True):
        return out(b, a.shape[1] + b.shape[1], b.shape[2], b.shape[3])

    return SimpleNamespace(conv_block=conv_block, conv_bn_block=conv_bn_block, down_bn_block=down_bn_block, res_bn_block=res_bn_block,
                           pool_bn_block=pool_bn_block, max_pool=max_pool, spp_concat=spp_concat, upsample_concat=upsample_concat)


def record_step(config):
    """The conv calls of one full-size training forward of ``config`` (a key of CONFIGS)."""
    import pytorch_yolo_amd as Y
    from pytorch_yolo_amd.models import train as MT
    import _cases as C
    cls, size, bs, anchors = CONFIGS[config]
    model = getattr(Y, cls)(n_class=80, anchors=getattr(C, anchors)).to("meta").train()
    calls = []
    p = MT.forward_train(model, torch.empty((bs, 3, size, size), dtype=F32, device="meta"), ops=recording_meta_ops(calls))
    assert len(p) == len(model.yolo_layers) and all(t.shape[0] == bs and t.shape[-1] == 85 for t in p)
    return calls


# ---- descriptors --------------------------------------------------------------------------------------------------------------------------
def forward_desc(n, h, w, cin, cout, k, stride=1, f32=False):
    """ops._desc of a training forward: the channels of x padded to 8 (ops._to_kernel_layout), act none (the batch norm follows; the
    plain heads have none either), bf16 out, or fp32 out with the row padded to 4 channels for a head."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_NONE, DT_BF16, DT_F32
    cin = K.roundup(cin, 8)
    return K.conv_desc(n=n, h=h, w=w, cin=cin, in_c_total=cin, in_c_offset=0, cout=cout, out_c_total=K.roundup(cout, 4) if f32 else cout,
                       out_c_offset=0, ksize=k, stride=stride, act=ACT_NONE, kpad=K.roundup(k * k * cin, 64), cout_pad=K.roundup(cout, 128),
                       out_dtype=DT_F32 if f32 else DT_BF16)


def dgrad_desc(d):
    """The descriptor yolo_conv2d_bwd_data (csrc/conv_bwd.hip) hands to the forward dispatcher for the forward's stride-1 ``d``: g
    [n, h, w, roundup(cout, 8)] in, the view of x out, act none, bf16."""
    from pytorch_yolo_amd import kernels as K
    from pytorch_yolo_amd._lib import ACT_NONE, DT_BF16
    cg = K.roundup(d.cout, 8)
    return K.conv_desc(n=d.n, h=d.h, w=d.w, cin=cg, in_c_total=cg, in_c_offset=0, cout=d.cin, out_c_total=d.in_c_total,
                       out_c_offset=d.in_c_offset, ksize=d.ksize, stride=1, act=ACT_NONE, kpad=K.roundup(d.ksize * d.ksize * cg, 64),
                       cout_pad=K.roundup(d.cin, 128), out_dtype=DT_BF16, pad=d.pad)


def family(pick):
    """A pick string without its grid(s), split count and per-class tile counts: the kernel and its tile."""
    return "; ".join(part.split(" grid ")[0].strip() for part in pick.split(";"))


def picks_of(d, need_dx=True):
    """{role: family} of one conv call with the forward descriptor ``d`` under the tuning words and compute-unit share in force."""
    from pytorch_yolo_amd import kernels as K
    out = {"forward": family(K.conv2d_pick(d))}
    if d.stride == 2:
        wgrad, dgrad = family(K.conv2d_down_bwd_pick(d)).split("; ")
        out["wgrad"] = wgrad
        if need_dx:
            out["dgrad_s2"] = dgrad
    else:
        out["wgrad"] = family(K.conv2d_bwd_pick(d))
        if need_dx:
            out["dgrad"] = family(K.conv2d_pick(dgrad_desc(d)))
    return out


def enumerate_step(config):
    """Counter of (role, family) over the conv calls of one training step of ``config``, and the calls as
    [(kind, layer (n, h, w, cin, cout, k), stride, {role: family})]."""
    count, rows = collections.Counter(), []
    for kind, xs, ws, stride, need_dx in record_step(config):
        n, cin, h, w = xs
        cout, _, k, _ = ws
        p = picks_of(forward_desc(n, h, w, cin, cout, k, stride, kind == "head"), need_dx)
        count.update(p.items())
        rows.append((kind, (n, h, w, cin, cout, k), stride, p))
    return count, rows


# the cost cap of a case's float64 restatement (tests/_conv_bwd.grads): elements of F.unfold(x, k) - 256 MiB per float64 copy, about four
# copies live at once - and multiply-accumulates of the layer
UNFOLD_CAP, MAC_CAP = 32 * 2 ** 20, 2.2e9


def partial_and_two_k_steps(fam, n, ho, wo, k_terms):
    """The conditions of tests/_exact_cases.py on the conv a family runs, read off its tile: more than one pixel tile, the last one partial
    (for the 16x16 and 20x20 tiles: in both directions), and at least two K steps; k_terms = k k cin of that conv."""
    m = n * ho * wo
    if fam.startswith("igemm<"):
        bm, bk = int(fam[6:].split("x")[0]), int(fam.split(",BK")[1].split(",")[0])
        return m > bm and m % bm != 0 and -(-k_terms // bk) >= 2
    if fam.startswith("halo<"):
        th, tw = (int(v) for v in fam[5:].split(",")[0].split("x"))
        return ho > th and wo > tw and ho % th != 0 and wo % tw != 0 and -(-k_terms // int(fam.split(",CK")[1].split(",")[0])) >= 2
    if fam.startswith("t20"):
        return ho > 20 and wo > 20 and ho % 20 != 0 and wo % 20 != 0 and k_terms >= 128
    if fam.startswith("stream1x1p<"):
        px = int(re.search(r",(\d+) px>", fam).group(1))
        return m > px and m % px != 0 and k_terms >= 128
    if fam.startswith("stream1x1<"):
        return m > 64 and m % 64 != 0 and k_terms >= 128
    raise ValueError(fam)


# ---- the case table -----------------------------------------------------------------------------------------------------------------------
def _c(n, h, w, cin, cout, k, stride=1, knob2=0, f32=False, why=""):
    """A case: a tests/_conv_bwd.py case (act none as in the training forward, plain views), the stride, the tuning words (knob 0, 1, 2)
    and, where a knob is set, why."""
    return dict(case=(n, h, w, cin, cout, k, "none", F32 if f32 else BF16, None, None), stride=stride, knobs=(-1, 0, knob2), why=why)


def case_desc(c):
    n, h, w, cin, cout, k, act, dt, view, oview = c["case"]
    return forward_desc(n, h, w, cin, cout, k, c["stride"], dt == F32)


def case_picks(c):
    """{role: family} of a case under its own tuning words."""
    from test_conv_exact_cpu import tuning
    with tuning(*c["knobs"]):
        return picks_of(case_desc(c))


def down_case(c):
    """The tests/_conv_down.py form of a stride-2 case."""
    n, h, w, cin, cout, k = c["case"][:6]
    assert c["stride"] == 2 and k == 3
    return (n, h, w, cin, cout, None)


_H128, _H64X2, _H64 = "halo<16x16,128 couts,CK64,1 halo buffers,16x16x32>", "halo<16x16,64 couts,CK64,2 halo buffers>", "halo<16x16,64 couts,CK32,1 halo buffers>"
_F_T20, _F_T20S2 = "t20v2<400px x 128 couts, 4 waves>", "t20s2<400px x 128 couts, 4 waves, parity planes>"
_G = "igemm<%s,16x16x32>"
_M32 = "igemm<%s,32x32x16>"
_WHY_T20 = ("the shipped rule hands a %s to the 20x20-tile kernel only on maps that fill the chip (family_shape_search.py: nothing inside the "
            "cost cap); T20_ALWAYS is the word tests/_exact_cases.py uses for the family; n = 2 so that an image boundary is crossed")

# The cheapest layer family_shape_search.py prints for each (role, family), by multiply-accumulates; one layer serves two entries where
# its other role is wanted too.  Two entries are not the cheapest on purpose: the data gradients whose cout is a concat width (768, the
# FPN concat -> 256 conv of YOLOv3-SPP at 40x40) and the SPP width (2048 -> 512 at 20x20), each on the smallest map that keeps the
# family of the full-size layer (--cin 768 / --cin 2048); 384 (the 80x80 concat) comes with the stream1x1p<K 384> forward.  The two
# layers under a tuning word are the search's cheapest with n = 2, and the data-gradient one with 64 couts instead of 32 (a whole
# 64-channel K chunk of g).  The figure beside a layer is its GMAC where that is 0.1 or more.
_HALO = _c(1, 79, 83, 64, 128, 3)                 # 0.48 GMAC; 5x6 tiles of 16x16, last row of 15, last column of 3
_HALO32 = _c(1, 79, 83, 32, 64, 3)                # 0.12
_N128_2ST = _c(4, 5, 7, 64, 96, 3)                # 140 pixels: two 128-row tiles
_N256X64 = _c(8, 5, 7, 96, 64, 1)                 # 280 pixels: two 256-row tiles
_D256X64 = _c(8, 5, 7, 64, 96, 1)
_N128_3ST = _c(7, 23, 25, 128, 192, 1)            # 0.10
_D128_3ST = _c(7, 23, 25, 192, 128, 1)            # 0.10
_LOADERS = _c(4, 5, 7, 64, 256, 3)
_D_LOADERS = _c(4, 5, 7, 256, 64, 3)
_SPP2048 = _c(4, 21, 23, 2048, 128, 1)            # 0.51: the data gradient has cout 2048, eight 256-wide tiles
_CAT768 = _c(7, 39, 41, 768, 128, 1)              # 1.10: the data gradient has cout 768, six 128-wide tiles
_N256X128 = _c(3, 113, 119, 64, 96, 1)            # 0.25
_STREAM64 = _c(3, 113, 119, 128, 64, 1)           # 0.33
_STREAM256 = _c(3, 113, 119, 256, 128, 1)         # 1.32
_STREAM384 = _c(3, 113, 119, 384, 128, 1)         # 1.98: the data gradient has cout 384, three 128-wide tiles
_N256X256 = _c(4, 49, 51, 128, 1024, 1)           # 1.31
_D256X256 = _c(4, 49, 51, 1024, 128, 1)           # 1.31
_N256X32 = _c(8, 5, 7, 64, 8, 1)
_GENERIC = _c(8, 5, 7, 8, 8, 3)                   # cin 8: the gather without whole 32-channel K chunks (the image layer, 3 -> 8 channels)
_HEAD128 = _c(4, 5, 7, 64, 255, 3, f32=True)      # the plain heads: fp32 out, 255 couts in a 256-channel row
_HEAD64 = _c(2, 5, 7, 128, 255, 1, f32=True)
_T20_FWD = _c(4, 37, 39, 32, 1024, 3)             # 1.70: 2x2 tiles of 20x20 per image, last row of 17, last column of 19; eight cout tiles
_T20_DGRAD = _c(2, 21, 23, 128, 64, 3, knob2=E.T20_ALWAYS, why=_WHY_T20 % "data gradient")
_T20S2 = _c(2, 41, 43, 32, 128, 3, stride=2, knob2=E.T20_ALWAYS, why=_WHY_T20 % "stride-2 layer")

FAMILY_CASES = {
    ("forward", _H128): _HALO,
    ("dgrad", _H64X2): _HALO,
    ("forward", _H64): _HALO32,
    ("dgrad", _M32 % "256x32,4x1 waves,BK32,2 stages"): _HALO32,
    ("forward", _G % "128x128,2x4 waves,BK64,2 stages"): _N128_2ST,
    ("dgrad", _M32 % "256x64,4x1 waves,BK32,2 stages"): _D256X64,
    ("forward", _M32 % "256x64,4x1 waves,BK32,2 stages"): _N256X64,
    ("forward", _G % "128x128,2x4 waves,BK64,3 stages"): _N128_3ST,
    ("dgrad", _G % "64x64,2x2 waves,BK64,2 stages"): _N128_3ST,
    ("dgrad", _G % "128x128,2x4 waves,BK64,3 stages"): _D128_3ST,
    ("forward", _G % "64x64,2x2 waves,BK64,2 stages"): _D128_3ST,
    ("forward", _G % "128x256,2x4 waves+4 loaders,BK64,3 stages"): _LOADERS,
    ("dgrad", _G % "128x256,2x4 waves+4 loaders,BK64,3 stages"): _D_LOADERS,
    ("dgrad", _G % "128x256,2x8 waves,BK64,3 stages"): _SPP2048,
    ("dgrad", _G % "128x128,2x4 waves,BK64,2 stages"): _CAT768,
    ("forward", _G % "256x128,4x2 waves,BK32,2 stages"): _N256X128,
    ("forward", "stream1x1<64 couts,K 128>"): _STREAM64,
    ("dgrad", _G % "256x128,4x2 waves,BK32,2 stages"): _STREAM64,
    ("forward", "stream1x1p<128 couts,K 256,80 px>"): _STREAM256,
    ("forward", "stream1x1p<128 couts,K 384,48 px>"): _STREAM384,
    ("forward", _G % "256x256,4x4 waves,BK64,2 stages"): _N256X256,
    ("dgrad", _G % "256x256,4x4 waves,BK64,2 stages"): _D256X256,
    ("forward", _M32 % "256x32,4x1 waves,BK32,2 stages"): _N256X32,
    ("forward", _M32 % "256x32,4x1 waves,BK32,2 stages,generic"): _GENERIC,
    ("forward", _M32 % "128x128,2x2 waves,BK64,2 stages"): _HEAD128,
    ("forward", _M32 % "64x64,2x2 waves,BK64,2 stages"): _HEAD64,
    ("forward", _F_T20): _T20_FWD,
    ("dgrad", _F_T20): _T20_DGRAD,
    ("forward", _F_T20S2): _T20S2,
}
# the distinct layers, in the table's order
CASES = list({id(c): c for c in FAMILY_CASES.values()}.values())
# the families of the weight gradient and of the stride-2 data gradient over the four steps: the kernel and its tile, not the grid.  Each
# is launched by the cases above (every case runs its weight gradient) or by tests/_conv_down.py (PICKS: both parity tiles, both wgrad tiles)
OTHER_FAMILIES = {("wgrad", "wgrad<64x128,BK64,tr_b16>"), ("wgrad", "wgrad<128x128,BK64,tr_b16>"), ("wgrad", "wgrad<64x128,BK64,tr_b16,s2>"),
                  ("wgrad", "wgrad<128x128,BK64,tr_b16,s2>"), ("dgrad_s2", "dgrad<128x64,BK64,parity>"), ("dgrad_s2", "dgrad<128x128,BK64,parity>")}


def layer_id(c):
    n, h, w, cin, cout, k = c["case"][:6]
    return f"{n}x{h}x{w}_{cin}to{cout}_k{k}_s{c['stride']}" + ("_f32" if c["case"][7] == F32 else "") + ("_knob" if c["knobs"] != (-1, 0, 0) else "")
