"""Pair-sharded relation-query across the GPUs of one node (RCCL over xGMI).

The reference has no inference parallelism (`assert batch_size == 1`, one GPU; V4:112,
openseed_relation_v2.py:93).  Object pairs are independent given the per-image constants, so they
shard naturally.  One process per GPU; a job is R images for R ranks (weak scaling):

  1. rank m patch-embeds image m and ALL-GATHERS its patches [L,256] fp32 (256 KB - not the
     67 MB feature map); every rank recomputes the tiny shared cross-attention K/V itself;
  2. for every image, rank r runs the Q-Former on the contiguous pair range
     [r*ceil(B/R), (r+1)*ceil(B/R)) and ALL-GATHERS the existence probabilities (40 KB at N=100);
  3. every rank runs the same deterministic top-K on the same gathered vector (no broadcast);
  4. the selected pair features (K x 32 x 768) live on whichever rank owned the pair: each rank
     fills a zero buffer with the rows it owns and a REDUCE-SCATTER(sum) hands image m's buffer to
     rank m (exactly one non-zero contributor per row, so the sum is exact);
  5. rank m decodes image m's K pairs (LLM weights replicated) and token ids are ALL-GATHERED.

`step_one_image` is the STRONG-scaling form (one image for all ranks, BASELINE C4): rank 0 - where the segmenter
ran - broadcasts the image's constants in ONE int32 message: object ids [N], object bitmasks [N, ceil(L/64)] and the
patch embedding [L, 256] (~260 KB instead of the 67 MB feature map).  The other ranks never see the image:
names and prompt ids follow from the object ids.  Every rank runs its pair shard, probabilities are all-gathered, the selected pair features are
all-reduced (one non-zero contributor per row) and the K decodes are DEALT round-robin to the ranks (SURVEY 8e
item 3; LLM weights replicated), token ids all-gathered.  What dealing can and cannot buy: a decode step streams
all 13.5 GB of Llama weights for 1 row as for 20, so only the compute-bound prompt pass and the relation query
shrink with the rank count; without tensor parallelism (out of scope) one image's latency is bounded
below by 16 weight passes.

Messages are <= 1 MB: latency-bound, so each step is one collective on the compute stream.
The compute is behind a small backend interface so the collective logic can be exercised with
`gloo` on CPU (tests/test_dist_gloo.py injects the CPU oracle); the product backend is
`HipBackend`, which drives the HIP head and has no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from ._lib import PsgHipError


def shard_range(num_pairs: int, world: int, rank: int):
    """Contiguous pair range of `rank` and the (uniform, padded) shard length."""
    shard = (num_pairs + world - 1) // world
    p0 = min(num_pairs, rank * shard)
    return p0, min(num_pairs, p0 + shard), shard


def shard_images(num_images: int, world: int, rank: int):
    """SURVEY 8e "replicas-only parts": whole images are dealt round-robin to ranks (C5)."""
    return list(range(rank, num_images, world))


def merge_image_results(parts, num_images: int):
    """parts[r] = [(image index, result)] of rank r -> the full list in image order; every image exactly once."""
    out = [None] * num_images
    for part in parts:
        for idx, res in part:
            if out[idx] is not None:
                raise RuntimeError(f"image {idx} was processed by two ranks")
            out[idx] = res
    missing = [i for i, r in enumerate(out) if r is None]
    if missing:
        raise RuntimeError(f"images {missing} were processed by no rank")
    return out


def gather_image_results(indexed_results, num_images: int, group=None, always_collective=False):
    """Every rank hands in [(image index, result)] for its share; every rank gets the full list in
    image order.  Results are host objects (numpy maps, python lists), so this is an object gather.
    always_collective: run the object gather at world size 1 too (first-run insurance for the RCCL path)."""
    import torch.distributed as dist
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1 and not (always_collective and dist.is_initialized()):
        parts = [indexed_results]
    else:
        parts = [None] * world
        dist.all_gather_object(parts, indexed_results, group=group)
    return merge_image_results(parts, num_images)


class HipBackend:
    """Adapter from the pipeline's compute calls to `RelationTransformerHeadV4` on one GPU."""

    def __init__(self, head):
        from .categories import INSTANCE_OFFSET, object_categories
        if getattr(head, "rel_cls_type", "binary") != "binary":
            # the multiclass scores of all pairs would need an all-gather of [pairs, R] and a global top-k merge
            raise PsgHipError(f"pair-sharded pipelines run rel_cls_type='binary' heads only, not {head.rel_cls_type!r} "
                              "(the multiclass head runs on one GPU: head.forward / submit / forward_batch)")
        if getattr(head, "llm_rel_scores", "constant") != "constant":
            raise PsgHipError("pair-sharded pipelines score LLM triples with the constant 1 only; "
                              "llm_rel_scores='likelihood' runs on one GPU (head.forward / submit)")
        if getattr(head, "llm_decode", "greedy") != "greedy":
            raise PsgHipError("pair-sharded pipelines run the free greedy decode only; llm_decode='constrained' runs on one "
                              "GPU (head.forward / submit / forward_batch)")
        self.head = head
        # the same object truncation (V4:136) and selector options as head.forward, so sharded == single GPU
        self._ids = lambda scene: [int(i) for i in scene["object_id_list"][:head.max_object_num]]
        self._names = lambda scene: [object_categories[i % INSTANCE_OFFSET] for i in self._ids(scene)]
        self.device = head.device
        self.feat_dtype = head.act_dtype
        self.q_rows = head.cfg.qformer.q_rows
        self.hidden = head.cfg.qformer.hidden
        self.max_new = head.cfg.max_new_tokens

    def num_objects(self, scene):
        return len(self._ids(scene))

    def patch_embed(self, scene):
        return self.head.rq_engine.patch_embed(scene["mask_features"].to(torch.float32))

    def image_constants(self, scene):
        """(object ids int32 [N], bitmasks int64 [N, W], patches fp32 [L, C]) of an image this rank holds."""
        ids = self._ids(scene)
        patches, bits = self.head.image_constants(scene["mask_features"], scene["img_meta"], ids, scene["pan_results"])
        return torch.tensor(ids, dtype=torch.int32, device=self.device), bits, patches

    def scene_from_ids(self, ids):
        """What a rank that received an image's constants knows of it: the object ids (names, prompts, decode)."""
        return dict(object_id_list=[int(i) for i in ids.tolist()])

    def query_shard(self, scene, patches, p0, p1, bits=None):
        if bits is not None:                          # constants of another rank: the image itself is not here
            rq = self.head.run_relation_query(None, None, self._ids(scene), self._names(scene), None, pair_range=(p0, p1),
                                              patches=patches, bits=bits)
            return (rq if "pending" in rq else rq["hidden"]), rq["exist_prob"]
        rq = self.head.run_relation_query(scene["mask_features"], scene["img_meta"], self._ids(scene), self._names(scene),
                                          scene["pan_results"], pair_range=(p0, p1), patches=patches)
        # cls-first head: the "hidden" handle is the pending selection-phase state (rows 1..32 are computed for the
        # selected pairs only, in gather_features)
        return (rq if "pending" in rq else rq["hidden"]), rq["exist_prob"]

    def query_shards(self, scenes, patches, ranges):
        """The shard ranges[m] = (p0, p1) of image m, all images in ONE Q-Former pass where the head can (per-image
        cross-attention only)."""
        items = [(s["mask_features"], s["img_meta"], self._ids(s), self._names(s), s["pan_results"]) for s in scenes]
        return self.head.run_relation_query_shards(items, list(ranges), [patches[m] for m in range(len(scenes))])

    def select(self, prob, num_objects):
        """The head's selector on the gathered probabilities: 'topk' (V4:235-237) or 'threshold' (the commented
        V4:230-234 logic; the count is data dependent, and identical on every rank because the input is)."""
        return self.head.select_pairs(prob, num_objects)      # honours exclude_diagonal (V4 never excludes)

    def gather_features(self, hidden, rows):
        from . import ops
        if isinstance(hidden, dict):                  # pending selection phase: rows = local pair * 33 + 1 + v, or -1
            nv = self.q_rows - 1
            r0 = rows.view(-1, nv)[:, 0].to(torch.int64)
            p0 = hidden["pair_range"][0]
            sel = torch.where(r0 >= 0, (r0 - 1) // self.q_rows + p0, torch.full_like(r0, -1))
            return self.head.selected_pair_features(hidden, sel, zero_foreign=True)
        out = torch.empty((rows.numel(), self.hidden), device=self.device, dtype=self.feat_dtype)
        if hidden.shape[0] == 0:                      # empty shard: nothing owned here
            return out.zero_()
        ops.gather_rows(hidden, rows, out)
        return out

    def gather_features_multi(self, hiddens, rows_list):
        """gather_features for every image of a step at once: handles of one selection-phase pass share their last
        layer (one pass over all images' selected pairs instead of one per image)."""
        if not all(isinstance(h, dict) for h in hiddens):
            return [self.gather_features(h, r) for h, r in zip(hiddens, rows_list)]
        nv = self.q_rows - 1
        sels = []
        for h, rows in zip(hiddens, rows_list):
            r0 = rows.view(-1, nv)[:, 0].to(torch.int64)
            sels.append(torch.where(r0 >= 0, (r0 - 1) // self.q_rows + h["pair_range"][0], torch.full_like(r0, -1)))
        return self.head.selected_pair_features_multi(hiddens, sels)

    def decode(self, scene, selected, features):
        rq = dict(num_objects=self.num_objects(scene))
        out = self.head.decode_selected(rq, self._names(scene), selected=selected, pair_features=features,
                                        to_host=False)
        return out["tokens"]

    def decode_dealt(self, scene, selected, features):
        """`decode` for a DEALT subset of an image's selected pairs (strong scaling): an fp32s head
        switches its prompt pass to the row-count-invariant projections, so that a pair decodes to the same bits in a
        batch of 3 on this rank as in the batch of 20 on one GPU (the single-GPU head gives those bits with
        `head.llm_engine.row_invariant = True`; with the library GEMM it is fp32-grade noise apart)."""
        eng = self.head.llm_engine
        prev = eng.row_invariant
        eng.row_invariant = prev or bool(eng.prefill_split)
        try:
            return self.decode(scene, selected, features)
        finally:
            eng.row_invariant = prev

    def decode_multi(self, scenes, selected_list, features_list):
        """The decodes of several images of this rank, side by side on the head's slot streams."""
        items = [dict(rq=dict(num_objects=self.num_objects(s)), names=self._names(s), selected=sel, pair_features=f)
                 for s, sel, f in zip(scenes, selected_list, features_list)]
        return [o["tokens"] for o in self.head.decode_concurrent(items)]


def deal_indices(k: int, world: int, rank: int):
    """Positions (into the selection) of the pairs rank `rank` decodes: round-robin."""
    return list(range(rank, k, world))


class LoopbackWorld:
    """R ranks inside ONE process (the single-process "fake world").  The pipelines below are written as
    generators that yield their collective requests; here the R rank generators advance in lockstep and every request
    is served from Python lists - all_gather / all_reduce / reduce_scatter / broadcast with the semantics of
    torch.distributed.  With `HipBackend` ranks sharing one head on one GPU this drives the whole sharded path -
    shard arithmetic, padding, selection, feature routing, dealt decodes - through the real kernels without a
    cluster (tests/test_gpu_fakeworld.py); the ranks run one after the other between two exchange points."""

    def __init__(self, world: int):
        self.world = int(world)

    def pipelines(self, backends, decode=True):
        """One PairShardedPipeline per rank; backends: one backend (shared by all ranks) or a list of R."""
        bes = backends if isinstance(backends, (list, tuple)) else [backends] * self.world
        return [PairShardedPipeline(bes[r], decode=decode, world=self.world, rank=r) for r in range(self.world)]

    def run(self, gens):
        """gens[r]: rank r's generator.  Returns the list of their return values."""
        R = self.world
        assert len(gens) == R
        results, reqs, sends, started = [None] * R, [None] * R, [None] * R, False
        while True:
            done = 0
            for r in range(R):                        # advance every rank to its next exchange point
                try:
                    reqs[r] = gens[r].send(sends[r]) if started else next(gens[r])
                except StopIteration as e:
                    results[r] = e.value
                    done += 1
            started = True
            if done:
                if done != R:
                    raise RuntimeError("ranks left the pipeline at different exchange points")
                return results
            kinds = {q[0] for q in reqs}
            if len(kinds) != 1:
                raise RuntimeError(f"ranks issued different collectives: {sorted(kinds)}")
            kind = kinds.pop()
            if kind == "all_gather":
                g = torch.stack([q[1].contiguous() for q in reqs])
                sends = [g] * R
            elif kind == "all_reduce":
                tot = reqs[0][1].clone()
                for q in reqs[1:]:
                    tot += q[1]
                sends = [tot.clone() for _ in range(R)]
            elif kind == "reduce_scatter":
                tot = reqs[0][1].clone()
                for q in reqs[1:]:
                    tot += q[1]
                sends = [tot[r].contiguous() for r in range(R)]
            elif kind == "broadcast":
                src = reqs[0][2]
                sends = [reqs[src][1]] * R
            else:
                raise RuntimeError(f"unknown collective {kind!r}")


class PairShardedPipeline:
    def __init__(self, head_or_backend, group=None, decode=True, world=None, rank=None):
        """world / rank given explicitly: a rank of a LoopbackWorld (no process group is touched; use the `*_gen`
        generators).  Otherwise the ranks of `group` (RCCL on GPUs, gloo in the CPU tests)."""
        self.be = head_or_backend if hasattr(head_or_backend, "query_shard") else HipBackend(head_or_backend)
        self.group = group
        if world is None:
            world, rank = dist.get_world_size(group), dist.get_rank(group)
        self.world, self.rank = int(world), int(rank)
        self.decode = decode

    # ---- the collectives behind a generator's requests ---------------------------------------------------------------
    def _all_gather(self, t):
        flat = t.contiguous().view(-1)
        out = torch.empty(self.world * flat.numel(), device=t.device, dtype=t.dtype)
        dist.all_gather_into_tensor(out, flat, group=self.group)
        return out.view((self.world,) + tuple(t.shape))

    def _reduce_scatter_sum(self, send):
        """send [R, ...] -> this rank's slice of the element-wise sum over ranks."""
        if dist.get_backend(self.group) == "gloo":          # CPU tests: gloo has no reduce_scatter
            tmp = send.clone()
            dist.all_reduce(tmp, op=dist.ReduceOp.SUM, group=self.group)
            return tmp[self.rank].contiguous()
        recv = torch.empty_like(send[0])
        dist.reduce_scatter_tensor(recv.view(-1), send.contiguous().view(-1), op=dist.ReduceOp.SUM, group=self.group)
        return recv

    _BCAST_DTYPES = (torch.float32, torch.int32, torch.int64, torch.float16, torch.bfloat16, torch.uint8)

    def _broadcast(self, t, src, device):
        """Two phases: shape + dtype (8 int64), then the payload."""
        g_src = dist.get_global_rank(self.group, src) if self.group is not None else src
        meta = torch.zeros(8, dtype=torch.int64, device=device)
        if self.rank == src:
            meta[0] = t.dim()
            for i, d in enumerate(t.shape):
                meta[1 + i] = d
            meta[7] = self._BCAST_DTYPES.index(t.dtype)
        dist.broadcast(meta, src=g_src, group=self.group)
        if self.rank != src:
            m = meta.tolist()
            t = torch.empty([int(x) for x in m[1:1 + int(m[0])]], device=device, dtype=self._BCAST_DTYPES[int(m[7])])
        dist.broadcast(t, src=g_src, group=self.group)
        return t

    def _drive(self, gen):
        """Runs a pipeline generator against the process group."""
        try:
            req = next(gen)
            while True:
                kind = req[0]
                if kind == "all_gather":
                    res = self._all_gather(req[1])
                elif kind == "all_reduce":
                    res = req[1]
                    if self.world > 1:
                        dist.all_reduce(res, op=dist.ReduceOp.SUM, group=self.group)
                elif kind == "reduce_scatter":
                    res = self._reduce_scatter_sum(req[1])
                elif kind == "broadcast":
                    res = req[1] if self.world == 1 else self._broadcast(req[1], req[2], req[3])
                else:
                    raise RuntimeError(f"unknown collective {kind!r}")
                req = gen.send(res)
        except StopIteration as e:
            return e.value

    def step_one_image(self, scene, deal_decodes=True):
        """Strong scaling: ONE image, its pairs sharded over all ranks; returns dict(exist_prob [B], selected [K],
        tokens [K, max_new]) identical on every rank."""
        return self._drive(self.step_one_image_gen(scene, deal_decodes))

    def step(self, scenes):
        """scenes[m] = inputs of image m, resident on every rank (object counts and image sizes may differ); P * world
        of them, image m owned by rank m % world.
        Returns dict with per-image lists: existence probabilities, selections and (if decoding) token ids."""
        return self._drive(self.step_gen(scenes))

    def _device(self, scene):
        if scene is not None and scene.get("mask_features") is not None:
            return scene["mask_features"].device
        return self.be.device

    @staticmethod
    def pack_constants(ids, bits, patches):
        """One int32 message: [N, W, L, C | ids (N) | bitmask words (2 N W) | patches (L C, fp32 bit patterns)]."""
        N, W = bits.shape
        L, C = patches.shape
        head = torch.tensor([N, W, L, C], dtype=torch.int32, device=patches.device)
        return torch.cat([head, ids.to(torch.int32).reshape(-1), bits.contiguous().view(torch.int32).reshape(-1),
                          patches.contiguous().view(torch.int32).reshape(-1)])

    @staticmethod
    def unpack_constants(msg):
        N, W, L, C = (int(v) for v in msg[:4].tolist())
        o = 4
        ids = msg[o:o + N].clone()
        o += N
        bits = msg[o:o + 2 * N * W].clone().view(torch.int64).reshape(N, W)
        o += 2 * N * W
        patches = msg[o:o + L * C].clone().view(torch.float32).reshape(L, C)
        return ids, bits, patches

    # ---- the pipelines, as generators yielding ("collective", tensor, ...) requests --------------------------------
    def step_one_image_gen(self, scene, deal_decodes=True):
        """scene: the image's inputs on rank 0 (where the segmenter ran); ignored - may be None - on every other rank,
        which works from rank 0's broadcast alone."""
        be, R, r = self.be, self.world, self.rank
        dev = self._device(scene)
        # 1. the image's constants from the rank that holds it: object ids, object bitmasks, patches - one message of
        #    ~260 KB instead of the 67 MB feature map and the full-resolution id map
        if hasattr(be, "image_constants"):
            msg = self.pack_constants(*be.image_constants(scene)) if r == 0 else None
            msg = yield ("broadcast", msg, 0, dev)
            ids, bits, patches = self.unpack_constants(msg)
            scene = scene if r == 0 else be.scene_from_ids(ids)
        else:                                                       # backends without mask kernels (the CPU test oracle)
            bits = None
            patches = be.patch_embed(scene) if r == 0 else None
            patches = yield ("broadcast", patches, 0, dev)
        N = be.num_objects(scene)
        B = N * N
        # 2. my pair shard; 3. probabilities everywhere, identical selection everywhere
        p0, p1, shard = shard_range(B, R, r)
        hidden, prob = be.query_shard(scene, patches, p0, p1) if bits is None else be.query_shard(scene, patches, p0, p1, bits)
        prob_pad = torch.full((shard,), -1.0, device=patches.device, dtype=torch.float32)
        prob_pad[:p1 - p0] = prob
        probs = (yield ("all_gather", prob_pad)).reshape(-1)[:B].contiguous()
        sel = be.select(probs, N)                                                    # K may be data dependent
        K = sel.numel()
        out = dict(exist_prob=probs, selected=sel)
        if not self.decode:
            return out
        # 4. features of the selected pairs to everyone (exactly one rank owns each row -> the sum is exact)
        nv = be.q_rows - 1
        s64 = sel.to(torch.int64)
        mine = (s64 >= p0) & (s64 < p1)
        rows = (s64 - p0)[:, None] * be.q_rows + 1 + torch.arange(nv, device=patches.device, dtype=torch.int64)[None, :]
        rows = torch.where(mine[:, None], rows, torch.full_like(rows, -1)).reshape(-1).to(torch.int32)
        feats = be.gather_features(hidden, rows)                                    # [K*nv, hidden], zeros where not mine
        feats = yield ("all_reduce", feats)
        # 5. the K decodes dealt round-robin; 6. token ids to everyone
        if deal_decodes and R > 1:
            per = (K + R - 1) // R
            idx = deal_indices(K, R, r)
            tok_pad = torch.full((per, be.max_new), -1, device=patches.device, dtype=torch.int32)
            if idx:
                it = torch.tensor(idx, device=patches.device, dtype=torch.int64)
                frow = (it[:, None] * nv + torch.arange(nv, device=patches.device)[None, :]).reshape(-1)
                tok_pad[:len(idx)] = getattr(be, "decode_dealt", be.decode)(scene, sel[it].contiguous(),
                                                                             feats[frow].contiguous())
            allt = yield ("all_gather", tok_pad)                                     # [R, per, max_new]
            tokens = torch.empty((K, be.max_new), device=patches.device, dtype=torch.int32)
            for rr in range(R):
                ii = deal_indices(K, R, rr)
                if ii:
                    tokens[torch.tensor(ii, device=patches.device)] = allt[rr, :len(ii)]
        else:
            tokens = be.decode(scene, sel, feats)
        out["tokens"] = tokens
        return out

    def step_gen(self, scenes):
        """P * R images per step, image m owned (patch-embedded and decoded) by rank m % R; P = 1 is SURVEY 8e's job of R
        images for R ranks.  With P > 1 a rank's P decodes run side by side on the head's slot streams
        (`decode_concurrent`: one image's row kernels under the other's weight streaming, as `head.submit` does on one
        GPU) - the collectives stay four per step, on the caller's stream."""
        be, R, r = self.be, self.world, self.rank
        assert len(scenes) and len(scenes) % R == 0, "a step is P images per rank: P * world scenes"
        n_img, P = len(scenes), len(scenes) // R
        Ns = [be.num_objects(s) for s in scenes]
        Bs = [n * n for n in Ns]
        # 1. patches of my images -> everyone (images of different sizes: padded to the longest patch list)
        ps = self._patch_size()
        Ls = [(s["mask_features"].shape[-2] // ps) * (s["mask_features"].shape[-1] // ps) for s in scenes]
        Lmax = max(Ls)
        mine = []
        for q in range(P):
            mp = be.patch_embed(scenes[q * R + r])
            assert mp.shape[0] == Ls[q * R + r]
            if mp.shape[0] < Lmax:
                mp = torch.cat([mp, mp.new_zeros((Lmax - mp.shape[0], mp.shape[1]))])
            mine.append(mp)
        allp = yield ("all_gather", torch.stack(mine))                              # [R, P, Lmax, C]
        patches = [allp[m % R, m // R, :Ls[m]].contiguous() for m in range(n_img)]
        dev = allp.device
        # 2. my pair shard of every image (the shard length depends on the image's object count)
        ranges = [shard_range(Bs[m], R, r) for m in range(n_img)]
        smax = max(1, max(rg[2] for rg in ranges))
        prob_pad = torch.full((n_img, smax), -1.0, device=dev, dtype=torch.float32)
        hidden = []
        if hasattr(be, "query_shards"):
            shards = be.query_shards(scenes, patches, [(rg[0], rg[1]) for rg in ranges])
        else:
            shards = [be.query_shard(scenes[m], patches[m], ranges[m][0], ranges[m][1]) for m in range(n_img)]
        for m, (h, prob) in enumerate(shards):
            hidden.append(h)
            prob_pad[m, :ranges[m][1] - ranges[m][0]] = prob
        gathered = yield ("all_gather", prob_pad)                                   # [rank, image, smax]
        probs = [gathered[:, m, :ranges[m][2]].reshape(-1)[:Bs[m]].contiguous() for m in range(n_img)]
        # 3. identical deterministic selection everywhere (K_m may be data dependent: threshold selector, tiny images)
        sel = [be.select(probs[m], Ns[m]) if Bs[m] else torch.zeros(0, dtype=torch.int32, device=dev)
               for m in range(n_img)]
        Ks = [int(s.numel()) for s in sel]
        out = dict(exist_prob=probs, selected=sel)
        if not self.decode:
            return out
        # 4. selected pair features -> the image's decoding rank
        nv = be.q_rows - 1
        Kmax = max(1, max(Ks))
        ar = torch.arange(nv, device=dev, dtype=torch.int64)
        rows_list = []
        for m in range(n_img):
            s = sel[m].to(torch.int64)
            p0, p1 = ranges[m][0], ranges[m][1]
            own = (s >= p0) & (s < p1)
            rows = (s - p0)[:, None] * be.q_rows + 1 + ar[None, :]               # pair_feature = hidden[:, 1:]
            rows_list.append(torch.where(own[:, None], rows, torch.full_like(rows, -1)).reshape(-1).to(torch.int32))
        live = [m for m in range(n_img) if Ks[m]]
        if hasattr(be, "gather_features_multi"):
            got = be.gather_features_multi([hidden[m] for m in live], [rows_list[m] for m in live])
        else:
            got = [be.gather_features(hidden[m], rows_list[m]) for m in live]
        send = torch.zeros((R, P, Kmax * nv, be.hidden), device=dev, dtype=got[0].dtype if got else torch.float32)
        for m, f in zip(live, got):
            send[m % R, m // R, :Ks[m] * nv] = f
        recv = yield ("reduce_scatter", send)                                      # [P, Kmax*nv, hidden] of MY images
        # 5. decode my images (side by side when there are several); 6. token ids to everyone
        tok_pad = torch.full((P, Kmax, be.max_new), -1, device=dev, dtype=torch.int32)
        todo = [q for q in range(P) if Ks[q * R + r]]
        if len(todo) > 1 and hasattr(be, "decode_multi"):
            toks = be.decode_multi([scenes[q * R + r] for q in todo], [sel[q * R + r] for q in todo],
                                   [recv[q, :Ks[q * R + r] * nv].contiguous() for q in todo])
        else:
            toks = [be.decode(scenes[q * R + r], sel[q * R + r], recv[q, :Ks[q * R + r] * nv].contiguous()) for q in todo]
        for q, t in zip(todo, toks):
            tok_pad[q, :Ks[q * R + r]] = t
        allt = yield ("all_gather", tok_pad)                                        # [R, P, Kmax, max_new]
        out["tokens"] = [allt[m % R, m // R, :Ks[m]].contiguous() for m in range(n_img)]
        return out

    def _patch_size(self):
        head = getattr(self.be, "head", None)
        return head.cfg.patch_size if head is not None else getattr(self.be, "patch_size", 16)
