"""PM-RoPE + KV-cache store (csrc/attn.hip rope_store_kernel) through t5g_rope_store, against
oracle/t5g_oracle.rope_cos_sin + apply_rope on CPU bf16 tensors with the same float positions
(non-integer, progress-scaled, up to 12 000; inv_freq = 10000^(-2i/D)).

Bit-equality, with one exception that is decided on the CPU before the comparison: the
device's cosf / sinf may differ from the host's by a few fp32 ulps, which changes a bf16 cos or
sin only where the true value lies next to a bf16 rounding tie. A (token, i) pair is *safe*
when its cos and its sin (fp64, of the fp32 angle) both lie more than 4 fp32 ulps from a tie:
every output of a safe pair must be bit-equal. An unsafe pair (8 of 65 536 fp32 values per
bf16 step and per trig value, so about 2^-12 of the pairs; at most 1 % is asserted) must equal
the reference recomputed with a neighbouring bf16 cos / sin. V rows and un-rotated heads are
copies. Every cache and Qout starts as a sentinel bit pattern, and every element the call
should not write must still hold it: a wrong slot, stride or row shows there.
"""
import ctypes as C

import pytest
import torch

from oracle.t5g_oracle import apply_rope, inv_freq_table, rope_cos_sin
from tests import kernel_cases as kc
from tests.engine_cases import need_gpu
from tests.kernel_cases import BF16, SENT
from tests.kernel_cases import bf16_step as _bf16_step
from tests.kernel_cases import i16 as _i16
from tests.kernel_cases import sentinel as _sentinel
from tests.kernel_cases import trig_safe as _trig_safe

pytestmark = pytest.mark.gpu


def _rot(x1, x2, c, s):
    """apply_rope's arithmetic on one rotation pair (bf16 tensor ops)."""
    return (x1 * c) + ((-x2) * s), (x2 * c) + (x1 * s)


class Case:
    """One t5g_rope_store call and its reference. lens: keys per row before the call's tokens
    are laid out; token m goes to row tok_row[m], slot tok_t[m]."""

    def __init__(self, seed, nq, nk, nv, D, lens, cap, rope_q=1, rope_k=1, col0=0, nsplit=0, decode=False,
                 inplace=False):
        g = torch.Generator().manual_seed(seed)
        self.nq, self.nk, self.nv, self.D, self.cap, self.B = nq, nk, nv, D, cap, len(lens)
        self.rope_q, self.rope_k, self.col0, self.nsplit, self.decode, self.inplace = rope_q, rope_k, col0, nsplit, decode, inplace
        nh = nq + nk + nv
        assert nk == nv   # the K and V caches share their strides
        if decode:   # one token per row at slot kv_len - 1, trig from the caller's table
            self.M, self.tok_row, self.tok_t, self.kv_len = len(lens), None, None, list(lens)
            rows = list(range(len(lens)))
        else:
            # tokens of the rows interleaved (packed order is not row order), slots from an offset
            toks = [(b, 2 * b + j) for b, L in enumerate(lens) for j in range(L)]
            perm = torch.randperm(len(toks), generator=g).tolist()
            toks = [toks[p] for p in perm]
            self.M, self.tok_row, self.tok_t = len(toks), [t[0] for t in toks], [t[1] for t in toks]
            self.kv_len = [1] * len(lens)   # must not be used
            rows = self.tok_row
        self.rows = rows
        M = self.M
        self.ldx = col0 + nh * D + 8
        self.ldq = self.ldx if inplace else nq * D + 16
        self.pos = (torch.rand(M, generator=g) * 12000.0).float()
        self.inv_freq = inv_freq_table(D, 10000.0)
        if nsplit:
            # slabs whose fp32 sum depends on the order (kernel_cases.order_slabs), added one by
            # one in fp32 in slab order, then rounded
            self.Xpart = kc.order_slabs(g, nsplit, M, self.ldx)
            self.X = kc.seq_sum(self.Xpart).to(BF16)
            self.order_sensitive = kc.order_sensitivity(self.Xpart)
        else:
            self.Xpart = None
            self.X = torch.randn(M, self.ldx, generator=g).to(BF16)
        # ---- reference
        cos, sin = rope_cos_sin(self.inv_freq, self.pos[None])       # bf16 [1][M][D]
        self.cos, self.sin = cos[0], sin[0]
        if decode:
            self.tab = torch.cat((self.cos[:, :D // 2], self.sin[:, :D // 2]), 1).float().contiguous()
            self.safe = torch.ones(M, D // 2, dtype=torch.bool)      # no device trig at all
        else:
            self.tab = None
            self.safe = _trig_safe(self.inv_freq, self.pos)
        xin = self.X[:, col0:col0 + nh * D].reshape(M, nh, D)
        rot = apply_rope(xin.transpose(0, 1)[None], cos, sin)[0].transpose(0, 1)   # [M][nh][D]
        self.rotated = torch.zeros(nh, dtype=torch.bool)
        self.rotated[:nq] = bool(rope_q)
        self.rotated[nq:nq + nk] = bool(rope_k)
        self.xin = xin
        self.ref = torch.where(self.rotated[None, :, None], rot, xin).contiguous()

    def run(self):
        """Launch; returns (Qbuf, Kc, Vc) host tensors ([M][ldq], [B][nk][cap][D], [B][nv][cap][D])."""
        from t5gemma_tts_amd import _lib
        dev = "cuda"
        D, cap = self.D, self.cap
        Xd = self.X.to(dev)
        Xp = self.Xpart.to(dev) if self.Xpart is not None else None
        Qd = Xd if self.inplace else _sentinel(self.M, self.ldq).to(dev)
        Kd = _sentinel(self.B, max(self.nk, 1), cap, D).to(dev)
        Vd = _sentinel(self.B, max(self.nv, 1), cap, D).to(dev)
        ti = lambda v: torch.tensor(v, dtype=torch.int32, device=dev) if v is not None else None
        trow, tt, kvl = ti(self.tok_row), ti(self.tok_t), ti(self.kv_len)
        posd, invd = self.pos.to(dev), self.inv_freq.to(dev)
        tabd = self.tab.to(dev) if self.tab is not None else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        a = _lib.RopeStoreArgs(X=None if Xp is not None else Xd.data_ptr(), Xpart=ptr(Xp), nsplit=self.nsplit,
                               ldx=self.ldx, M=self.M, D=D, nq=self.nq, nk=self.nk, nv=self.nv, col0=self.col0,
                               rope_q=self.rope_q, rope_k=self.rope_k, pos=posd.data_ptr(), inv_freq=invd.data_ptr(),
                               tok_row=ptr(trow), tok_t=ptr(tt), kv_len=kvl.data_ptr(),
                               Qout=Qd.data_ptr() if self.nq else None, ldq=self.ldq,
                               Kc=Kd.data_ptr() if self.nk else None, Vc=Vd.data_ptr() if self.nv else None,
                               c_bstride=max(self.nk, 1) * cap * D, c_hstride=cap * D, rope_tab=ptr(tabd))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().t5g_rope_store(C.byref(a), st), "rope_store")
        torch.cuda.synchronize()
        return Qd.cpu(), Kd.cpu(), Vd.cpu()

    def check(self, Qb, Kc, Vc, label):
        """Gather what the call wrote, check the sentinel everywhere else, compare."""
        M, D, nq, nk, nv = self.M, self.D, self.nq, self.nk, self.nv
        got = torch.empty(M, nq + nk + nv, D, dtype=BF16)
        if nq:
            got[:, :nq] = Qb[:, :nq * D].reshape(M, nq, D)
            rest = _i16(Qb).clone()
            if self.inplace:   # the other columns of X are as they were
                rest[:, :nq * D] = _i16(self.X)[:, :nq * D]
                assert torch.equal(rest, _i16(self.X)), "in-place q changed another column of X"
            else:
                assert (rest[:, nq * D:] == SENT).all(), "Qout written past the q heads"
        slots = {}
        for m in range(M):
            b = self.rows[m]
            slot = self.tok_t[m] if self.tok_t is not None else self.kv_len[b] - 1
            assert (b, slot) not in slots
            slots[(b, slot)] = m
        for cache, h0, n in ((Kc, nq, nk), (Vc, nq + nk, nv)):
            written = torch.zeros(cache.shape[:3], dtype=torch.bool)
            for (b, slot), m in slots.items():
                if n:
                    got[m, h0:h0 + n] = cache[b, :n, slot]
                    written[b, :n, slot] = True
            assert (_i16(cache)[~written] == SENT).all(), f"{label}: a cache slot outside the call's tokens was written"
        same = _i16(got) == _i16(self.ref)                       # [M][nh][D]
        H2 = D // 2
        pair_ok = same[..., :H2] & same[..., H2:]                 # [M][nh][D/2]
        copies = ~self.rotated
        assert pair_ok[:, copies].all(), f"{label}: a copied head (V or un-rotated) is not a bit-exact copy"
        safe = self.safe[:, None, :].expand_as(pair_ok)
        assert pair_ok[safe].all(), (label, "safe pairs not bit-equal", int((~pair_ok & safe).sum()))
        # unsafe pairs that differ: a neighbouring bf16 cos and / or sin must explain them
        bad = (~pair_ok & ~safe).nonzero().tolist()
        for m, h, i in bad:
            x1, x2 = self.xin[m, h, i], self.xin[m, h, i + H2]
            g1, g2 = _i16(got[m, h, i]).item(), _i16(got[m, h, i + H2]).item()
            hit = False
            for dc in (0, 1, -1):
                for ds in (0, 1, -1):
                    o1, o2 = _rot(x1, x2, _bf16_step(self.cos[m, i], dc), _bf16_step(self.sin[m, i], ds))
                    hit |= (_i16(o1).item(), _i16(o2).item()) == (g1, g2)
            assert hit, (label, "unsafe pair not explained by a neighbouring bf16 trig value", m, h, i)
        share = 1.0 - self.safe.float().mean().item()
        print(f"{label}: {M} tokens, unsafe pair share {share:.2e} ({int((~self.safe).sum())} of {self.safe.numel()}), "
              f"unsafe pairs that differ {len(bad)}, bit-equal outputs {same.float().mean().item():.6f}")
        assert share <= 0.01
        return share


ENC_LENS = [11, 1, 25]   # 37 tokens over 3 ragged rows


@pytest.mark.parametrize("inplace", [False, True], ids=["separate_q", "in_place_q"])
def test_encoder_shape(inplace):
    """nq 8, nk 4, nv 4, D 256: 37 tokens over 3 ragged rows in packed (shuffled) order, slots
    from tok_t, a cache larger than every row; q to its own buffer, and in place."""
    need_gpu()
    c = Case(1, 8, 4, 4, 256, ENC_LENS, 32, inplace=inplace)
    c.check(*c.run(), label=f"encoder inplace={inplace}")


def test_in_place_q_needs_one_stride():
    """Qout == X with ldq != ldx is refused before anything is launched."""
    need_gpu()
    from t5gemma_tts_amd import _lib
    x = torch.zeros(4, 4096, dtype=BF16, device="cuda")
    i = torch.zeros(4, dtype=torch.int32, device="cuda")
    f = torch.zeros(128, dtype=torch.float32, device="cuda")
    kc = _sentinel(1, 4, 8, 256).to("cuda")
    a = _lib.RopeStoreArgs(X=x.data_ptr(), ldx=4096, M=4, D=256, nq=8, nk=4, nv=4, rope_q=1, rope_k=1,
                           pos=f.data_ptr(), inv_freq=f.data_ptr(), tok_row=i.data_ptr(), tok_t=i.data_ptr(),
                           kv_len=i.data_ptr(), Qout=x.data_ptr(), ldq=2048, Kc=kc.data_ptr(), Vc=kc.data_ptr(),
                           c_bstride=4 * 8 * 256, c_hstride=8 * 256)
    assert _lib.lib().t5g_rope_store(C.byref(a), None) == _lib.T5G_EINVAL
    torch.cuda.synchronize()
    assert (_i16(kc.cpu()) == SENT).all() and not x.any()


def test_cross_kv_shape():
    """The prefill's cross K / V store: no q heads, rope on k only."""
    need_gpu()
    c = Case(2, 0, 4, 4, 256, [60, 1, 33], 70, rope_q=0, rope_k=1)
    c.check(*c.run(), label="cross k/v")


def test_unrotated_heads_are_copies():
    """rope_q = rope_k = 0: everything is a copy into the right place."""
    need_gpu()
    c = Case(3, 8, 4, 4, 256, ENC_LENS, 32, rope_q=0, rope_k=0)
    c.check(*c.run(), label="no rope")


def test_tiny_config():
    """D 64 with nq 2, nk 1, nv 1: 128 rotation pairs, half of the one 256-thread block idle."""
    need_gpu()
    c = Case(4, 2, 1, 1, 64, [7, 1, 12], 24)
    c.check(*c.run(), label="tiny")


def test_column_offset():
    """col0 = 2048: the k | v heads of q | k | v rows, the q heads left alone."""
    need_gpu()
    c = Case(5, 0, 4, 4, 256, ENC_LENS, 32, col0=2048)
    c.check(*c.run(), label="col0 2048")
    c = Case(6, 2, 1, 1, 64, [5, 3], 9, col0=40)
    c.check(*c.run(), label="col0 40, D 64")


@pytest.mark.parametrize("nsplit", [1, 3, 8])
def test_split_k_slabs(nsplit):
    """X as fp32 split-K slabs: summed in slab order in fp32, rounded to bf16, then rotated. The
    slab values make the sum depend on the order (two large slabs that cancel exactly first)."""
    need_gpu()
    c = Case(10 + nsplit, 8, 4, 4, 256, ENC_LENS, 32, nsplit=nsplit)
    if nsplit > 2:
        print(f"nsplit={nsplit}: {c.order_sensitive:.3f} of the bf16 sums differ when the slabs are added in reverse")
        assert c.order_sensitive >= 0.25
    c.check(*c.run(), label=f"Xpart nsplit={nsplit}")


def test_decode_form():
    """tok_row / tok_t null: token m is row m, slot kv_len[m] - 1; cos / sin from the caller's
    table, so no device trig and the whole output is bit-equal."""
    need_gpu()
    c = Case(20, 8, 4, 4, 256, [1, 17, 32, 5, 9], 32, decode=True)
    Qb, Kc, Vc = c.run()
    share = c.check(Qb, Kc, Vc, label="decode form")
    assert share == 0.0
    assert torch.equal(_i16(Kc[2, :, 31]), _i16(c.ref[2, 8:12]))   # the last slot of a full row
