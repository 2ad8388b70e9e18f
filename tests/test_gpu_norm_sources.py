"""resid_norm_kernel (csrc/norm.hip) through t5g_resid_norm_src, where t5g_resid_norm does not
go: the embedding-gather and split-K-slab sources, block widths from one wave to the
1 024-thread block, absent post_w / resid / pre_w (the host's stand-in pointers), out_rows
compaction and the side-written RoPE table. Reference and bounds are those of
tests/test_gpu_gemv.py test_resid_norm_vs_fp32: the fp32 restatement _rms, <= 2 bf16 ulps
everywhere and more than 95 % bit-equal. What no norm touches (a gathered, summed or copied
row) must be bit-exact. Every output buffer carries one extra row of a sentinel bit pattern
that must survive the call.
"""
import ctypes as C
import itertools

import pytest
import torch

from oracle.t5g_oracle import inv_freq_table
from tests import kernel_cases as kc
from tests.engine_cases import need_gpu
from tests.kernel_cases import BF16, EPS, SENT
from tests.kernel_cases import bf16_step as _bf16_step
from tests.kernel_cases import i16 as _i16
from tests.kernel_cases import rms_norm as _rms
from tests.kernel_cases import sentinel as _sentinel
from tests.kernel_cases import trig_safe as _trig_safe

pytestmark = pytest.mark.gpu


def _case(seed, M, d, src="delta", nsplit=0, post=True, resid=True, pre=True, want_h=True, out_rows=None,
          rope_D=0):
    """Run one call; returns (got_h or None, got_xn or None, ref_h, ref_xn or None, extras)."""
    from t5gemma_tts_amd import _lib
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    Ms = M if out_rows is None else 33            # source rows
    sel = list(range(M)) if out_rows is None else out_rows
    keep = []                                     # device tensors alive until the sync
    extras = {}
    a = _lib.NormSrcArgs(M=M, d=d, eps=EPS)

    def up(t):
        keep.append(t.to(dev))
        return keep[-1].data_ptr()

    if src == "delta":
        v = (torch.randn(Ms, d, generator=g) * 3.0).to(BF16)
        a.delta = up(v)
    elif src == "ids":
        table = torch.randn(300, d, generator=g).to(BF16)
        ids = torch.randint(0, 300, (Ms,), generator=g).tolist()
        ids[0], ids[-1] = 299, 0
        scale = torch.tensor(float(d) ** 0.5).to(BF16).item()    # the normalizer is a bf16 value
        a.ids, a.table, a.n_table, a.scale = up(torch.tensor(ids, dtype=torch.int32)), up(table), 300, scale
        v = (table[ids].float() * scale).to(BF16)
    else:
        ldp = d + 24
        p = kc.order_slabs(g, nsplit, Ms, ldp, amp=3.0)
        a.part, a.nsplit, a.ldp = up(p), nsplit, ldp
        v = kc.seq_sum(p)[:, :d].to(BF16)
        extras["order_sensitive"] = kc.order_sensitivity(p[:, :, :d])
    v = v[sel]
    post_w = (torch.randn(d, generator=g) * 0.1).to(BF16)
    pre_w = (torch.randn(d, generator=g) * 0.1).to(BF16)
    h_in = torch.randn(Ms, d, generator=g).to(BF16)
    if post:
        a.post_w = up(post_w)
        v = _rms(v, post_w)
    if resid:
        a.resid = up(h_in)
        v = (h_in[sel].float() + v.float()).to(BF16)
    ref_h, ref_xn = v, None
    hd = _sentinel(M + 1, d).to(dev)
    xd = _sentinel(M + 1, d).to(dev)
    if want_h:
        a.resid_out = hd.data_ptr()
    if pre:
        a.pre_w, a.normed_out = up(pre_w), xd.data_ptr()
        ref_xn = _rms(ref_h, pre_w)
    if out_rows is not None:
        a.out_rows = up(torch.tensor(out_rows, dtype=torch.int32))
    if rope_D:
        pos = (torch.rand(M, generator=g) * 12000.0).float()
        inv = inv_freq_table(rope_D, 10000.0)
        tab = torch.full((M + 1, rope_D), float("nan"), device=dev)
        a.rope_pos, a.rope_inv_freq, a.rope_tab, a.rope_D = up(pos), up(inv), tab.data_ptr(), rope_D
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().t5g_resid_norm_src(C.byref(a), st), "resid_norm_src")
    torch.cuda.synchronize()
    hc, xc = hd.cpu(), xd.cpu()
    assert (_i16(hc)[M] == SENT).all() and (_i16(xc)[M] == SENT).all(), "a row past M was written"
    if not want_h:
        assert (_i16(hc) == SENT).all()
    if not pre:
        assert (_i16(xc) == SENT).all()
    if rope_D:
        extras.update(pos=pos, inv=inv, tab=tab.cpu())
    return (hc[:M] if want_h else None), (xc[:M] if pre else None), ref_h, ref_xn, extras


def _close(pairs, label, exact_first=False):
    """test_resid_norm_vs_fp32's bounds on each (got, ref) pair, as there; exact_first: the first
    pair went through no norm and must be bit-exact."""
    for k, (got, ref) in enumerate(pairs):
        diff = (got.float() - ref.float()).abs()
        ulp = ref.float().abs().clamp(min=2.0 ** -20) * 2 ** -7
        worst, same = (diff / ulp).max().item(), (diff == 0).float().mean().item()
        print(f"{label} [output {k}]: worst error {worst:.2f} bf16 ulps (bound 2), bit-equal {same:.4f} "
              f"(bound > 0.95)")
        if exact_first and k == 0:
            assert torch.equal(_i16(got), _i16(ref)), f"{label}: the un-normed rows are not bit-exact"
        assert worst <= 2.0, (label, k)
        assert same > 0.95, (label, k)


@pytest.mark.parametrize("d", [8, 128, 2304, 8192])
@pytest.mark.parametrize("M", [1, 5, 33])
def test_widths(M, d):
    """d = 8, 128, 2304, 8192: 63, 48, 32 and 0 idle threads in blocks of 64, 64, 320 and 1 024;
    the full residual + two-norm form on the delta source."""
    need_gpu()
    h, xn, rh, rxn, _ = _case(d + M, M, d)
    _close([(h, rh), (xn, rxn)], f"delta M={M} d={d}")


@pytest.mark.parametrize("d", [8, 128, 2304, 8192])
def test_ids_source(d):
    """v = bf16(table[ids[m]] * scale) from a table of 300 rows (in-range ids, first and last
    row among them): as the layer-0 embedding launch (no post norm, no residual: h is the
    scaled row itself, bit-exact), and in the full form."""
    need_gpu()
    h, xn, rh, rxn, _ = _case(100 + d, 5, d, src="ids", post=False, resid=False)
    _close([(h, rh), (xn, rxn)], f"ids embed d={d}", exact_first=True)
    h, xn, rh, rxn, _ = _case(200 + d, 33, d, src="ids")
    _close([(h, rh), (xn, rxn)], f"ids full d={d}")


@pytest.mark.parametrize("nsplit", list(range(1, 9)))
def test_part_source(nsplit):
    """v = bf16(part[0] + part[1] + ...) over fp32 slabs with ldp > d, added in slab order in
    fp32: with no post norm and no residual, h is that sum, bit-exact, on values whose sum
    depends on the order. Then the full form."""
    need_gpu()
    for M, d in ((5, 2304), (33, 8), (3, 8192)):
        h, xn, rh, rxn, ex = _case(300 + nsplit + d, M, d, src="part", nsplit=nsplit, post=False, resid=False)
        if nsplit > 2:   # teeth, from the reference alone: the launch's own slabs, added in reverse, give other bits
            assert ex["order_sensitive"] >= 0.25, ex["order_sensitive"]
        _close([(h, rh), (xn, rxn)], f"part sum nsplit={nsplit} M={M} d={d}", exact_first=True)
    h, xn, rh, rxn, _ = _case(400 + nsplit, 5, 2304, src="part", nsplit=nsplit)
    _close([(h, rh), (xn, rxn)], f"part full nsplit={nsplit}")


@pytest.mark.parametrize("d", [8, 2304])
def test_absent_operands(d):
    """Every combination of post_w / resid / pre_w present or absent that resid_norm() accepts:
    all eight with resid_out, and the four with pre_w where only normed_out is written."""
    need_gpu()
    n = 0
    for post, resid, pre, want_h in itertools.product((True, False), repeat=4):
        if not want_h and not pre:
            continue   # nothing to write: refused
        for src in ("delta", "ids"):
            h, xn, rh, rxn, _ = _case(500 + n, 5, d, src=src, post=post, resid=resid, pre=pre, want_h=want_h)
            pairs = ([(h, rh)] if want_h else []) + ([(xn, rxn)] if pre else [])
            _close(pairs, f"{src} d={d} post={post} resid={resid} pre={pre} resid_out={want_h}",
                   exact_first=want_h and not post and not resid)
            n += 1
    assert n == 24


def test_out_rows():
    """A subset of 33 source rows, written compact: the source, the ids and resid are read at
    the source row, the outputs written at the compact row. Also the engine's gather form
    (delta source, nothing else: a bit-exact row copy)."""
    need_gpu()
    rows = [31, 0, 7, 32, 16]
    for src in ("delta", "ids"):
        h, xn, rh, rxn, _ = _case(600, 5, 2304, src=src, out_rows=rows)
        _close([(h, rh), (xn, rxn)], f"out_rows {src}")
    h, xn, rh, rxn, _ = _case(601, 5, 2304, out_rows=rows, post=False, resid=False, pre=False)
    assert xn is None and torch.equal(_i16(h), _i16(rh))
    h, xn, rh, rxn, _ = _case(602, 5, 8, out_rows=rows)
    _close([(h, rh), (xn, rxn)], "out_rows d=8")


@pytest.mark.parametrize("M,d,rope_D", [(5, 2304, 256), (33, 8, 256), (5, 8192, 64)])
def test_side_written_rope_table(M, d, rope_D):
    """Row i's block also writes bf16(cos) | bf16(sin) of rope_inv_freq * rope_pos[i] into
    rope_tab[i] (d = 8: 64 threads loop over 128 frequencies). Against fp64 cos / sin of the
    fp32 angle, with tests/test_gpu_rope_store.py's safe-set rule: bit-equal where cos and sin
    are more than 4 fp32 ulps from a bf16 tie, a neighbouring bf16 value elsewhere."""
    need_gpu()
    h, xn, rh, rxn, ex = _case(700 + d, M, d, rope_D=rope_D)
    _close([(h, rh), (xn, rxn)], f"rope side output M={M} d={d}")
    tab = ex["tab"]
    assert torch.isnan(tab[M]).all() and not torch.isnan(tab[:M]).any()
    ang = (ex["pos"][:, None] * ex["inv"][None, :]).double()
    ref = torch.cat((ang.cos(), ang.sin()), 1).to(BF16)
    safe = _trig_safe(ex["inv"], ex["pos"])
    safe2 = torch.cat((safe, safe), 1)
    got = tab[:M]
    assert torch.equal(got, got.to(BF16).float()), "table entries are bf16 values"
    same = got.to(BF16) == ref
    assert same[safe2].all(), int((~same & safe2).sum())
    for m, j in (~same & ~safe2).nonzero().tolist():
        near = {_bf16_step(ref[m, j], s).float().item() for s in (1, -1)}
        assert got[m, j].item() in near, (m, j)
    share = 1.0 - safe.float().mean().item()
    print(f"rope table M={M} D={rope_D}: unsafe pair share {share:.2e}, entries off the reference "
          f"{int((~same).sum())} of {same.numel()}")
    assert share <= 0.01
