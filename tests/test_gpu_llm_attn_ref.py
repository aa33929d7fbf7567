"""The LLM stage's attention kernels against float64 (`-m gpu`): llm_attn_kernel (psg_llm_attn(_gqa)), the four-wave and
the one-wave decode kernels (psg_decode_attn, option decode_attn_1wave), decode_attn_gqa_kernel (every split of a group),
the matrix-core prompt kernels and the fp32 one (psg_prefill_attn(_gqa)), the fused rope form
(psg_prefill_attn_rope(_gqa)) and tree_attn_kernel (psg_tree_attn), each compared with the restatements of
tests/llm_attn_ref.py under the bound derived there, elementwise, on plain random inputs and on the four directed
families (ascending_maximum, descending_maximum, last_key_matters, probability_rounding_edge).

Conventions: cache slots nobody has written hold NaN; padding rows of q / qkv hold finite junk of magnitude 2^10; every
output buffer is filled with a sentinel and has spare rows.  Asserted in every case: |got - ref| <= bound for every
element, padding rows exactly zero where the kernel writes them (the decode and trie kernels leave them alone), no cache
slot other than the appended ones changes a bit, and the appended K / V rows hold exactly the float64 rotation (exact on
these inputs) and the stored V.  Inputs of the fused kernels are the exact-rotation inputs of the reference module; the
decode cases need one pair per row (a row appends to its pair's cache).

Measured on an MI355X (100 tests, about 6 s wall time for the file, the float64 references included), worst err / bound:

    kernel                      fp32    bf16    fp16
    llm_attn                    0.011   0.980   0.889
    decode_attn (four-wave)     0.013   0.980   0.895
    decode_attn (one-wave)      0.013   0.980   0.895
    decode_attn_gqa             0.013   0.982   0.948
    prefill_attn                0.010   0.820   0.818
    prefill_attn_rope           -       0.820   0.818
    tree_attn                   0.011   0.989   0.944

The ratios above 0.95 (bf16 of every kernel that keeps fp32 probabilities) are near misses by construction, not by
accident: there the bound is u |ref| plus an fp32 term a hundred times smaller, and a correctly rounded output whose
exact value lies next to a rounding tie is off by almost exactly u |ref|.  The term that dominates is u |ref|.

What the file is known to catch (mutated copies of the library, never committed; each run of this file failed):
a truncating probability pack in the matrix-core prompt kernels (test_prefill_attn, test_prefill_attn_rope: 16-bit,
S >= 15, worst 1.26 on probability_rounding_edge); `key < qi` for the last key tile (S in 33, 63, 64 of the three prompt
tests); `alpha` left off the running output of llm_attn_kernel (every test_llm_attn); the padding-key mask dropped in the
rope form (only test_prefill_attn_rope_padding_between_real_rows: with padding at the end the causal mask hides every
padding key already); the one-wave decode kernel's 8-key tail skipping its last key (every test_decode_attn[*-one_wave]);
key / value head h % kvh for h // G (test_llm_attn[*-2], the 16-bit test_prefill_attn).  Before the matrix-core prompt
kernel selected zeros for its padding rows, every 16-bit test_prefill_attn failed: the pair without a real token
gathers V from a cache row nobody wrote, and 0 x NaN is NaN.
"""
import functools
import types

import pytest
import torch

from tests import llm_attn_ref as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = -1234.5
WORST = {}


def _note(kernel, dtype, ratio):
    WORST[(kernel, dtype)] = max(WORST.get((kernel, dtype), 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst err / bound per kernel and dtype: " + ", ".join(f"{k} {d} {v:.3f}" for (k, d), v in sorted(WORST.items())))


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _nan(shape, dt):
    return torch.full(shape, float("nan")).to(dt)


def _out(rows, cols, dt):
    return torch.full((rows + 5, cols), SENTINEL, device=DEV, dtype=dt)


def _spare_untouched(buf, rows):
    assert bool((buf[rows:] == SENTINEL).all()), "rows past the output were written"


def _same_bits(tag, got, want, signed_zero=True):
    """signed_zero=False (rotated keys): a zero may carry either sign - 0 * cos - 0 * sin has the sign the operation
    order gives it; everything else, the NaN of an unwritten slot included, bit for bit"""
    got = got.cpu()
    if not signed_zero:
        got, want = (torch.where(t == 0, torch.zeros_like(t), t) for t in (got, want))
    assert torch.equal(_bits(got), _bits(want)), f"{tag}: bits differ"


# ---- prompt blocks: psg_prefill_attn(_gqa) and psg_prefill_attn_rope(_gqa) on one case ----
BLOCK_S = [1, 15, 16, 17, 31, 32, 33, 63, 64]
HEADS = 4


@functools.lru_cache(maxsize=None)
def _prompt_case(dtype, S, G, family, holes=False):
    """Four pairs of S rows with S, S - 1, 1 and NO real token; the stored q and caches of the plain form, the qkv rows of
    the fused form (which must produce exactly those caches) and one float64 reference for both.  holes (the fused form
    only, S >= 4): rows 2 and S // 2 + 1 of the first two pairs are padding as well.  With padding at the end only, a
    padding key is above the diagonal of every real row and the causal mask hides it already; a padding row between real
    ones is the only place where the key mask itself decides.  (The plain form reads its keys from the first `real
    count` cache rows and does not take such a block.)"""
    dt = DT[dtype]
    g = torch.Generator().manual_seed(1000 * S + 10 * G + L.FAMILIES.index(family))
    kvh = HEADS // G
    lens = [S, S - 1, 1, 0]
    pairs, ctx, rows = len(lens), S + 3, len(lens) * S
    cos, sin = L.exact_rope_tables(ctx, g)
    qrot = torch.zeros(pairs, S, HEADS, 128, dtype=torch.float64)
    krot = torch.zeros(pairs, S, kvh, 128, dtype=torch.float64)
    for p in range(pairs):
        for hk in range(kvh):
            qrot[p, :, hk * G:(hk + 1) * G], krot[p, :, hk] = L.family_qk(family, S, S, G, dt, g)
    v = L.family_v(family, (pairs, kvh, S, 128), g).to(dt)                      # [pair][kv head][key]
    real = torch.tensor([[t < n for t in range(S)] for n in lens])
    if holes:
        real[:2, 2] = False
        real[:2, S // 2 + 1] = False
    tok_pos = torch.where(real, torch.arange(S)[None, :], torch.tensor(-1)).reshape(-1).to(torch.int32)
    q = torch.where(real[:, :, None], qrot.reshape(pairs, S, -1), L.junk((pairs, S, HEADS * 128), g)).reshape(rows, -1).to(dt)
    kc, vc = _nan((pairs, kvh, ctx, 128), dt), _nan((pairs, kvh, ctx, 128), dt)
    for p in range(pairs):
        kc[p][:, :S][:, real[p]] = krot[p, real[p]].transpose(0, 1).to(dt)
        vc[p][:, :S][:, real[p]] = v[p][:, real[p]]
    pos = torch.arange(S).repeat(pairs)
    xq = L.unrotate(qrot.reshape(rows, HEADS, 128), pos, cos, sin).reshape(rows, -1)
    xk = L.unrotate(krot.reshape(rows, kvh, 128), pos, cos, sin).reshape(rows, -1)
    xv = v.double().permute(0, 2, 1, 3).reshape(rows, -1)
    W = (HEADS + 2 * kvh) * 128
    qkv = torch.where(real.reshape(rows, 1), torch.cat([xq, xk, xv], 1), L.junk((rows, W), g)).to(dt)
    assert float(qkv[real.reshape(-1)][:, :(HEADS + kvh) * 128].double().abs().max()) <= 4.0      # q, k inside the grid
    ref, A, gx, n, sv = L.causal64(q, kc, vc, tok_pos, pairs, S, HEADS, sum_v=True)
    return types.SimpleNamespace(dt=dt, kvh=kvh, pairs=pairs, ctx=ctx, rows=rows, rope=(cos, sin), q=q, kc=kc, vc=vc,
                                 qkv=qkv, tok_pos=tok_pos, real=real.reshape(-1), ref=ref, A=A, gx=gx, n=n, sv=sv)


def _group(S, family):
    return (1, 2, 4)[(BLOCK_S.index(S) + L.FAMILIES.index(family)) % 3]


def _check_block(tag, c, buf, p_rounded, kernel, dtype):
    _spare_untouched(buf, c.rows)
    got = buf[:c.rows].cpu()
    assert bool((got[~c.real] == 0).all()), f"{tag}: a padding row is not exactly zero"
    bound = L.attn_bound(c.ref, c.A, c.gx, c.n, c.dt, p_rounded=p_rounded, sum_v=c.sv)
    _note(kernel, dtype, L.check(tag, got, c.ref, bound))


@pytest.mark.parametrize("S", BLOCK_S)
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_prefill_attn(dtype, S):
    from openpsg_amd import ops
    for family in L.FAMILIES:
        G = _group(S, family)
        c = _prompt_case(dtype, S, G, family)
        kd, vd = c.kc.to(DEV), c.vc.to(DEV)
        buf = _out(c.rows, HEADS * 128, c.dt)
        ops.prefill_attn(c.q.to(DEV), kd, vd, c.tok_pos.to(DEV), c.pairs, S, HEADS, 128, c.ctx, buf[:c.rows],
                         kv_heads=c.kvh if G > 1 else None)
        torch.cuda.synchronize()
        tag = f"prefill_attn {dtype} S={S} G={G} {family}"
        _check_block(tag, c, buf, dtype != "fp32", "prefill_attn", dtype)
        _same_bits(tag + " K cache", kd, c.kc)
        _same_bits(tag + " V cache", vd, c.vc)


@pytest.mark.parametrize("S", BLOCK_S)
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_prefill_attn_rope(dtype, S):
    from openpsg_amd import ops
    for family in L.FAMILIES:
        G = _group(S, family)
        c = _prompt_case(dtype, S, G, family)
        kd, vd = _nan(c.kc.shape, c.dt).to(DEV), _nan(c.kc.shape, c.dt).to(DEV)
        buf = _out(c.rows, HEADS * 128, c.dt)
        ops.prefill_attn_rope(c.qkv.to(DEV), c.tok_pos.to(DEV), (c.rope[0].to(DEV), c.rope[1].to(DEV)), c.pairs, S, HEADS, 128,
                              c.ctx, kd, vd, buf[:c.rows], kv_heads=c.kvh if G > 1 else None)
        torch.cuda.synchronize()
        tag = f"prefill_attn_rope {dtype} S={S} G={G} {family}"
        _check_block(tag, c, buf, True, "prefill_attn_rope", dtype)
        # the K rows written are exactly the float64 rotation, the V rows the stored ones; padding tokens' rows stay NaN
        _same_bits(tag + " K cache", kd, c.kc, signed_zero=False)
        _same_bits(tag + " V cache", vd, c.vc)


@pytest.mark.parametrize("S", [s_ for s_ in BLOCK_S if s_ >= 4])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_prefill_attn_rope_padding_between_real_rows(dtype, S):
    from openpsg_amd import ops
    for family in ("random", "last_key_matters"):
        G = _group(S, family)
        c = _prompt_case(dtype, S, G, family, holes=True)
        kd, vd = _nan(c.kc.shape, c.dt).to(DEV), _nan(c.kc.shape, c.dt).to(DEV)
        buf = _out(c.rows, HEADS * 128, c.dt)
        ops.prefill_attn_rope(c.qkv.to(DEV), c.tok_pos.to(DEV), (c.rope[0].to(DEV), c.rope[1].to(DEV)), c.pairs, S, HEADS, 128,
                              c.ctx, kd, vd, buf[:c.rows], kv_heads=c.kvh if G > 1 else None)
        torch.cuda.synchronize()
        tag = f"prefill_attn_rope (padding between real rows) {dtype} S={S} G={G} {family}"
        _check_block(tag, c, buf, True, "prefill_attn_rope", dtype)
        _same_bits(tag + " K cache", kd, c.kc, signed_zero=False)
        _same_bits(tag + " V cache", vd, c.vc)


# ---- psg_llm_attn(_gqa): one wave per (row, head), keys [0, pos] ----
POS = [0, 1, 62, 63, 64, 65, 127, 128, 129, 191]


@functools.lru_cache(maxsize=None)
def _prefix_case(dtype, G, family):
    """Two pairs with 192 cached keys; a row per position of POS and pair, plus one padding row: 21 rows, and 3 or 6 heads
    for G = 1, 2 (rows * heads no multiple of the 4 waves of a workgroup), 4 heads for G = 4."""
    dt = DT[dtype]
    g = torch.Generator().manual_seed(77 + 10 * G + L.FAMILIES.index(family))
    heads = {1: 3, 2: 6, 4: 4}[G]
    kvh, pairs, nk, ctx = heads // G, 2, 192, 195
    rows = pairs * len(POS) + 1
    order = torch.randperm(rows, generator=g)
    tok_pair = torch.tensor([p for p in range(pairs) for _ in POS] + [1], dtype=torch.int32)[order]
    tok_pos = torch.tensor(POS * pairs + [-1], dtype=torch.int32)[order]
    q = L.junk((rows, heads, 128), g)
    kc, vc = _nan((pairs, kvh, ctx, 128), dt), _nan((pairs, kvh, ctx, 128), dt)
    for p in range(pairs):
        mine = ((tok_pair == p) & (tok_pos >= 0)).nonzero().flatten()
        for hk in range(kvh):
            q_, k_ = L.family_qk(family, nk, len(mine), G, dt, g, window=nk, kmax=4.0)
            q[mine, hk * G:(hk + 1) * G] = q_
            kc[p, hk, :nk] = k_.to(dt)
    vc[:, :, :nk] = L.family_v(family, (pairs, kvh, nk, 128), g).to(dt)
    q = q.reshape(rows, -1).to(dt)
    ref, A, gx, n = L.prefix64(q, kc, vc, tok_pair, tok_pos, heads)
    return types.SimpleNamespace(dt=dt, heads=heads, kvh=kvh, ctx=ctx, rows=rows, q=q, kc=kc, vc=vc, tok_pair=tok_pair,
                                 tok_pos=tok_pos, ref=ref, A=A, gx=gx, n=n)


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_llm_attn(dtype, G):
    from openpsg_amd import ops
    for family in L.FAMILIES:
        c = _prefix_case(dtype, G, family)
        kd, vd = c.kc.to(DEV), c.vc.to(DEV)
        buf = _out(c.rows, c.heads * 128, c.dt)
        ops.llm_attn(c.q.to(DEV), kd, vd, c.tok_pair.to(DEV), c.tok_pos.to(DEV), c.heads, 128, c.ctx, buf[:c.rows],
                     kv_heads=c.kvh if G > 1 else None)
        torch.cuda.synchronize()
        tag = f"llm_attn {dtype} G={G} {family}"
        _spare_untouched(buf, c.rows)
        got = buf[:c.rows].cpu()
        assert bool((got[c.tok_pos < 0] == 0).all()), f"{tag}: the padding row is not exactly zero"
        _note("llm_attn", dtype, L.check(tag, got, c.ref, L.attn_bound(c.ref, c.A, c.gx, c.n, c.dt)))
        _same_bits(tag + " K cache", kd, c.kc)
        _same_bits(tag + " V cache", vd, c.vc)


# ---- the decode step: psg_decode_attn (four-wave unit, one-wave kernel) and psg_decode_attn_gqa ----
# cached keys before the new token: the one-wave kernel's P.V tails of 32 / 8 / 1 keys (40 = 32 + 8, 47 = 32 + 8 + 7,
# 104 = 64 + 32 + 8) and the four-wave kernel's 16 keys per wave (15 / 16 / 17, 31 / 32 / 33, 47, 63 / 64 / 65)
COUNTS = (0, 1, 7, 8, 15, 16, 17, 31, 32, 33, 40, 47, 63, 64, 65, 96, 104, 129, 199)
GQA_COUNTS = {2: (0, 1, 8, 16, 17, 33, 47, 63, 64, 96, 199), 4: (0, 7, 15, 31, 32, 40, 65, 104, 129),
              8: (1, 16, 17, 32, 40, 64, 65, 129, 199)}


@functools.lru_cache(maxsize=None)
def _decode_case(dtype, heads, kvh, family, counts, splits):
    """A row (and a pair) per cached-key count plus one padding row; exact-rotation q / k of the new token, the cached
    keys as stored, split-K input as grid partials (then the new token's v sits on the grid too)."""
    dt = DT[dtype]
    g = torch.Generator().manual_seed(5000 + 100 * heads + 10 * kvh + 3 * splits + L.FAMILIES.index(family))
    G = heads // kvh
    rows, ctx = len(counts) + 1, 203
    order = torch.randperm(rows, generator=g)
    pos = torch.tensor(list(counts) + [-1], dtype=torch.int32)[order]
    pair = torch.randperm(rows, generator=g).to(torch.int32)
    cos, sin = L.exact_rope_tables(ctx, g)
    qrot = torch.zeros(rows, heads, 128, dtype=torch.float64)
    knew = torch.zeros(rows, kvh, 128, dtype=torch.float64)
    vnew = torch.zeros(rows, kvh, 128, dtype=torch.float64)
    kc, vc = _nan((rows, kvh, ctx, 128), dt), _nan((rows, kvh, ctx, 128), dt)
    for r in range(rows):
        n = int(pos[r])
        if n < 0:
            continue
        v = L.family_v(family, (kvh, n + 1, 128), g)
        if splits:
            v[:, n] = torch.round(v[:, n] * 16) / 16 + 0.0         # (+ 0.0: a sum of partials is never -0)
        v = v.to(dt)
        vc[int(pair[r]), :, :n], vnew[r] = v[:, :n], v[:, n].double()
        for hk in range(kvh):
            q_, k_ = L.family_qk(family, n + 1, 1, G, dt, g)
            qrot[r, hk * G:(hk + 1) * G], knew[r, hk] = q_[0], k_[n]
            kc[int(pair[r]), hk, :n] = k_[:n].to(dt)
    live = pos >= 0
    p0 = pos.clamp(min=0).long()
    x = torch.cat([L.unrotate(qrot, p0, cos, sin).reshape(rows, -1), L.unrotate(knew, p0, cos, sin).reshape(rows, -1),
                   vnew.reshape(rows, -1)], 1)
    x = torch.where(live[:, None], x, L.junk(tuple(x.shape), g))
    qkv = L.split_exact(x, splits, g) if splits else x.to(dt)
    assert torch.equal((qkv.sum(0) if splits else qkv).double(), x)
    ref, A, gx, n = L.decode64(qrot, knew, vnew, kc, vc, pair, pos, heads)
    kc2, vc2 = kc.clone(), vc.clone()                              # the caches after the step
    for r in range(rows):
        if pos[r] >= 0:
            kc2[int(pair[r]), :, int(pos[r])] = knew[r].to(dt)
            vc2[int(pair[r]), :, int(pos[r])] = vnew[r].to(dt)
    return types.SimpleNamespace(dt=dt, heads=heads, kvh=kvh, ctx=ctx, rows=rows, rope=(cos, sin), qkv=qkv, splits=splits,
                                 pair=pair, pos=pos, live=live, kc=kc, vc=vc, kc2=kc2, vc2=vc2, ref=ref, A=A, gx=gx, n=n)


def _run_decode(tag, c, kernel, dtype):
    from openpsg_amd import ops
    kd, vd = c.kc.to(DEV), c.vc.to(DEV)
    buf = _out(c.rows, c.heads * 128, c.dt)
    x = ops.Partials(c.qkv.to(DEV).contiguous()) if c.splits else c.qkv.to(DEV)
    ops.decode_attn(x, c.pair.to(DEV), c.pos.to(DEV), (c.rope[0].to(DEV), c.rope[1].to(DEV)), c.heads, 128, c.ctx, kd, vd,
                    buf[:c.rows], kv_heads=c.kvh if c.kvh != c.heads else None)
    torch.cuda.synchronize()
    _spare_untouched(buf, c.rows)
    got = buf[:c.rows].cpu()
    pad = got[~c.live]
    assert bool((pad == 0).all()) or bool((pad == SENTINEL).all()), f"{tag}: the padding row holds neither zeros nor its old bits"
    bound = L.attn_bound(c.ref, c.A, c.gx, c.n, c.dt)
    _note(kernel, dtype, L.check(tag, got[c.live], c.ref[c.live], bound[c.live]))
    _same_bits(tag + " K cache after the step", kd, c.kc2, signed_zero=False)
    _same_bits(tag + " V cache after the step", vd, c.vc2)


@pytest.mark.parametrize("unit", ["four_wave", "one_wave"])
@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_decode_attn(dtype, splits, unit):
    from openpsg_amd import _lib
    old = _lib.get_option(0, "decode_attn_1wave")
    try:
        _lib.set_option(0, "decode_attn_1wave", 1 if unit == "one_wave" else 0)
        for family in L.FAMILIES:
            c = _decode_case(dtype, 2, 2, family, COUNTS, splits)
            _run_decode(f"decode_attn {unit} {dtype} splits={splits} {family}", c, "decode_attn_" + unit, dtype)
    finally:
        _lib.set_option(0, "decode_attn_1wave", old)


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_decode_attn_gqa(dtype, G):
    from openpsg_amd import _lib
    old = _lib.get_option(0, "decode_gqa_qparts")
    try:
        for family in L.FAMILIES:
            splits = 3 if family in ("random", "ascending_maximum") else 0
            c = _decode_case(dtype, 8, 8 // G, family, GQA_COUNTS[G], splits)
            for qparts in (0, 1, 2, 4, 8):
                if qparts > G:
                    continue
                _lib.set_option(0, "decode_gqa_qparts", qparts)
                _run_decode(f"decode_attn_gqa {dtype} G={G} qparts={qparts} splits={splits} {family}", c, "decode_attn_gqa",
                            dtype)
    finally:
        _lib.set_option(0, "decode_gqa_qparts", old)


# ---- psg_tree_attn ----
PREFIX = (0, 1, 63, 64, 65, 125)                                   # + depth 1 .. 8: key counts cross 64 and 128
TRIE_BASE, MAX_DEPTH = 130, 8
# parent of every trie node (a parent precedes its children): a chain of depth 8 (nodes 0 .. 7), roots 8 and 11
PARENT = (-1, 0, 1, 2, 3, 4, 5, 6, -1, 8, 8, -1, 0, 12)


@functools.lru_cache(maxsize=None)
def _tree_case(dtype, heads, kvh, family):
    dt = DT[dtype]
    g = torch.Generator().manual_seed(900 + 10 * heads + kvh + 100 * L.FAMILIES.index(family))
    G, n_int, pairs = heads // kvh, len(PARENT), len(PREFIX)
    anc = torch.full((n_int, MAX_DEPTH), -1, dtype=torch.int32)
    for i in range(n_int):
        chain, a = [], i
        while a >= 0:
            chain.append(a)
            a = PARENT[a]
        anc[i, :len(chain)] = torch.tensor(chain[::-1], dtype=torch.int32)
    ctx = TRIE_BASE + n_int + 2
    row_pair = torch.arange(pairs, dtype=torch.int32).repeat_interleave(n_int)
    row_node = torch.arange(n_int, dtype=torch.int32).repeat(pairs)
    row_pair = torch.cat([row_pair, torch.tensor([-1, 2], dtype=torch.int32)])     # two rows the kernel must skip
    row_node = torch.cat([row_node, torch.tensor([3, -1], dtype=torch.int32)])
    rows = row_pair.numel()
    q = L.junk((rows, heads, 128), g)
    kc, vc = _nan((pairs, kvh, ctx, 128), dt), _nan((pairs, kvh, ctx, 128), dt)
    for p, plen in enumerate(PREFIX):
        slots = list(range(plen)) + list(range(TRIE_BASE, TRIE_BASE + n_int))      # key order: prompt, then nodes by id
        vc[p][:, slots] = L.family_v(family, (kvh, len(slots), 128), g).to(dt)
        for hk in range(kvh):
            q_, k_ = L.family_qk(family, len(slots), n_int, G, dt, g, window=len(slots), kmax=4.0)
            q[p * n_int:(p + 1) * n_int, hk * G:(hk + 1) * G] = q_
            kc[p, hk, slots] = k_.to(dt)
    q = q.reshape(rows, -1).to(dt)
    live = (row_pair >= 0) & (row_node >= 0)
    plen_t = torch.tensor(PREFIX, dtype=torch.int32)
    ref, A, gx, n = L.tree64(q[live], kc, vc, row_pair[live], row_node[live], plen_t, anc, TRIE_BASE, heads)
    assert sorted(set(n.tolist())) [0] == 1 and {64, 65, 128, 129} <= set(n.tolist())
    return types.SimpleNamespace(dt=dt, ctx=ctx, rows=rows, q=q, kc=kc, vc=vc, row_pair=row_pair, row_node=row_node,
                                 plen=plen_t, anc=anc, live=live, ref=ref, A=A, gx=gx, n=n)


@pytest.mark.parametrize("heads,kvh", [(4, 4), (4, 2), (8, 1)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_tree_attn(dtype, heads, kvh):
    from openpsg_amd import ops
    for family in L.FAMILIES:
        c = _tree_case(dtype, heads, kvh, family)
        kd, vd = c.kc.to(DEV), c.vc.to(DEV)
        buf = _out(c.rows, heads * 128, c.dt)
        ops.tree_attn(c.q.to(DEV), kd, vd, c.row_pair.to(DEV), c.row_node.to(DEV), c.plen.to(DEV), c.anc.to(DEV), TRIE_BASE,
                      heads, 128, c.ctx, buf[:c.rows], kv_heads=kvh)
        torch.cuda.synchronize()
        tag = f"tree_attn {dtype} heads={heads} kv={kvh} {family}"
        _spare_untouched(buf, c.rows)
        got = buf[:c.rows].cpu()
        skipped = got[~c.live]
        assert bool((skipped == 0).all()) or bool((skipped == SENTINEL).all()), f"{tag}: a skipped row was written"
        bound = L.attn_bound(c.ref, c.A, c.gx, c.n, c.dt)
        _note("tree_attn", dtype, L.check(tag, got[c.live], c.ref, bound))
        _same_bits(tag + " K cache", kd, c.kc)
        _same_bits(tag + " V cache", vd, c.vc)
