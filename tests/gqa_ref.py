"""Float64 restatement of grouped-query attention (GQA) for the kernel tests: rotary on the stored values, every query
head h attending key / value head h // G through `repeat_interleave`, softmax in float64.  Shared by
tests/test_gpu_gqa_kernels.py and tests/test_gpu_gqa_head.py."""
import torch


def rope_tables(ctx, theta=10000.0, hd=128):
    """cos / sin fp32 tables [ctx, hd / 2] as the engine builds them (llm.py, HF-LL:115-128)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(ctx, dtype=torch.float32)[:, None] * inv_freq[None, :]
    return ang.cos().contiguous(), ang.sin().contiguous()


def rope64(x, pos, cos, sin):
    """Half-split rotary of x [rows, n, 128] (float64) at table rows `pos` (int [rows], >= 0)."""
    c = cos.double()[pos][:, None, :]
    s = sin.double()[pos][:, None, :]
    x1, x2 = x[..., :64], x[..., 64:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def split_qkv(qkv, heads, kv_heads):
    """[rows, (heads + 2 kv) 128] -> q [rows, heads, 128], k, v [rows, kv, 128]."""
    rows = qkv.shape[0]
    D, Dk = heads * 128, kv_heads * 128
    return (qkv[:, :D].reshape(rows, heads, 128), qkv[:, D:D + Dk].reshape(rows, kv_heads, 128),
            qkv[:, D + Dk:].reshape(rows, kv_heads, 128))


def attend64(q, kc, vc, pairs, nkeys):
    """q [rows, heads, 128] float64; caches [P, kv, ctx, 128] float64; row r attends keys [0, nkeys[r]) of its pair
    pairs[r] (nkeys[r] <= 0: zeros).  Returns [rows, heads * 128]."""
    rows, heads = q.shape[:2]
    G = heads // kc.shape[1]
    out = torch.zeros((rows, heads, 128), dtype=torch.float64)
    for r in range(rows):
        n = int(nkeys[r])
        if n <= 0:
            continue
        k = kc[int(pairs[r]), :, :n].repeat_interleave(G, dim=0)          # [heads, n, 128]
        v = vc[int(pairs[r]), :, :n].repeat_interleave(G, dim=0)
        s = torch.einsum("hd,hnd->hn", q[r], k) / 128 ** 0.5
        out[r] = torch.einsum("hn,hnd->hd", torch.softmax(s, dim=-1), v)
    return out.reshape(rows, heads * 128)


def expand_kv_rows(w_kv, G):
    """A key / value projection weight [kv 128, hidden] as the multi-head weight [kv G 128, hidden]: head j's 128 rows
    repeated G times in place (query heads j G .. j G + G - 1 read it)."""
    kv = w_kv.shape[0] // 128
    return w_kv.view(kv, 1, 128, -1).expand(-1, G, -1, -1).reshape(kv * G * 128, -1).contiguous()
