"""`RelationTransformerHeadV4`: MI355X-native drop-in for the reference relation head.

Mirrors kings_sgg/models/relation_heads/relation_transformer_head_v4.py (V4): same registry name
(V4:20-21), same constructor keywords (V4:22-45), same `forward(inputs: dict) -> dict` contract in
eval mode (inputs `mask_features`, `img_metas`, `object_info` as packed by
openseed_relation_v2.py:177-181; outputs `rel_pred`, `rel_score`, V4:355-356), same state-dict
names so a reference checkpoint loads with `strict=False`
(part_checkpoint_hook.py:96-116 drops `language_model.*`).

Differences that are deliberate and documented:
  * V4:355-356 raises UnboundLocalError in the default 'binary' mode as committed; this head
    implements the intended contract: rel_pred = LLM triples, rel_score = 1 each;
  * the training branch computes the reference's two losses (`forward_train`: values through the inference kernels;
    `forward_train_grad`: with the gradient graph, fp32 or train_precision='bf16' - openpsg_amd/train_graph.py);
  * rel_cls_type 'binary+multiclass' / 'multiclass' (V4:31, 91-95): the multiclass triples follow the LLM triples with
    the diagonal zeroed and the flat index decoded as p*R + r (V4:239-250 as intended), and 'multiclass' alone runs no
    pair selector or decode;
  * all arithmetic runs in libpsg_hip.so / hipBLASLt on the GPU; there is no CPU path.
"""
from __future__ import annotations

import weakref

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._lib import PsgHipError
from .categories import INSTANCE_OFFSET, object_categories, relation_categories
from .config import REL_CLS_TYPES, LlamaConfig, PSGConfig, QFormerConfig
from .llm import LlamaDecodeEngine
from .qformer import RelationQueryEngine
from .registry import HEADS
from .rel_scores import MAX_RANKED_TRIPLES, assemble, build_relation_trie
from .tokenizers import WordTokenizer
from .weights import (head_shapes, hf_checkpoint_has_weights, is_hf_checkpoint_dir, llm_quant_keys, llm_shapes,
                      read_hf_llama_config, read_hf_llama_weights)

_DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32, "float32": torch.float32,
           "fp16": torch.float16, "float16": torch.float16, "half": torch.float16, "mixed": torch.float16,
           "mixed_q32": torch.float16, "fp32s": torch.float32,
           torch.bfloat16: torch.bfloat16, torch.float32: torch.float32, torch.float16: torch.float16}


class _Pending:
    """An image submitted with `head.submit`: its kernels are enqueued on `stream`; `result()` is the only host wait."""

    def __init__(self, head, stream, rq, out, num_objects, inputs=None, slot=None):
        self.head, self.stream, self.rq, self.out, self.N, self.slot = head, stream, rq, out, num_objects, slot
        # the caller's input tensors are read on `stream`, possibly long after `submit` returned: they stay referenced
        # here until the result is taken (and carry a record_stream mark in case the handle is dropped first)
        self.inputs = inputs
        self._result = None

    def result(self):
        if self._result is not None:                                  # taken before: the same dict again
            return self._result
        if self.rq is None:
            self._result = dict(rel_pred=[], rel_score=[])
            return self._result
        h, out = self.head, self.out
        with torch.cuda.stream(self.stream):
            sel = self.rq["selected"]
            if out.get("tokens") is None and "_finish" not in out:         # 'multiclass' alone: no decode
                out["tokens_host"] = out["selected_host"] = None
            if out.get("beam_class") is not None:                          # llm_beam_width > 1: classes and scores, no tokens
                out["beam_class_host"], out["beam_logp_host"] = out["beam_class"].cpu().numpy(), out["beam_logp"].cpu().numpy()
                out["selected_host"] = sel.cpu().numpy()
            if "_finish" in out:                                           # natural EOS: the chunks behind the first
                out.pop("_finish")()
                # the deferred chunks were enqueued only now: `_decode_done` of this image (recorded at submit, behind the
                # first chunk) must cover them, or `serialize_decodes` / `_wait_front` would let the next decode start early
                if h._decode_done_slot == self.slot:
                    h._decode_done = torch.cuda.Event()
                    h._decode_done.record(self.stream)
            if out["tokens"] is not None:
                out["tokens_host"] = out["tokens"].cpu().numpy()           # waits for this stream's work only
                out["selected_host"] = sel.cpu().numpy()
                if out.get("rel_logscores") is not None:
                    out["logscores_host"] = out["rel_logscores"].cpu().numpy()
                if out.get("path_logp") is not None:
                    out["path_logp_host"] = out["path_logp"].cpu().numpy()
            if h.has_multiclass:
                out["mc_host"] = self.rq["mc_topk"].cpu().numpy()
        self.rq.update(out)
        h.last = self.rq
        decoded = out["tokens_host"] is not None or out.get("beam_class_host") is not None
        rel_pred, rel_score = h._parse_out(out, self.N) if decoded else ([], [])
        mc_pred, mc_score = h.parse_multiclass(out.get("mc_host"), self.N)
        self.rq = self.out = self.inputs = None
        self._result = dict(rel_pred=rel_pred + mc_pred, rel_score=rel_score + mc_score)
        return self._result

    @property
    def taken(self):
        return self._result is not None


class _PendingBatch:
    """A batch submitted with `head.submit_batch`; `result()` is the only host wait (on the batch's stream)."""

    def __init__(self, head, stream, items, results, tokens, mcs=None):
        self.head, self.stream, self.items, self.results, self.tokens = head, stream, items, results, tokens
        self.mcs = mcs or {}                                    # image -> (multiclass top-k [2, k] on the device, N)

    def result(self):
        h, results = self.head, self.results
        if not self.items and not self.mcs:
            return results
        with torch.cuda.stream(self.stream):
            tokens_host = self.tokens.cpu().numpy() if self.items else None
            sels = [sel.cpu().numpy() for _, _, sel, _, _ in self.items]
            mc_host = {i: t.cpu().numpy() for i, (t, _) in self.mcs.items()}
        k0 = 0
        h.last_batch = []
        for (i, N, _, X, _), sel_host in zip(self.items, sels):
            k1 = k0 + X.shape[0]
            rel_pred, rel_score = h.parse(tokens_host[k0:k1], sel_host, N)
            results[i] = dict(rel_pred=rel_pred, rel_score=rel_score)
            h.last_batch.append(dict(tokens_host=tokens_host[k0:k1], selected_host=sel_host))
            k0 = k1
        for i, (_, N) in self.mcs.items():                      # V4:355-356: LLM triples, then the multiclass ones
            mc_pred, mc_score = h.parse_multiclass(mc_host[i], N)
            r = results[i] if results[i] is not None else dict(rel_pred=[], rel_score=[])
            results[i] = dict(rel_pred=r["rel_pred"] + mc_pred, rel_score=r["rel_score"] + mc_score)
        self.items = self.tokens = None
        self.mcs = {}
        return results


def _set_nested(root: nn.Module, dotted: str, tensor: torch.Tensor):
    parts = dotted.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, nn.Module())
        mod = mod._modules[p]
    mod.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=False))


class _LazyRQ(dict):
    """Relation-query result of the cls-first path: `hidden` (the last layer's 33 rows of EVERY pair) is not part
    of the inference path any more; a reader that asks for it (tests, tools) gets it computed on demand."""
    engine = None

    def __missing__(self, key):
        if key != "hidden":
            raise KeyError(key)
        hs = [self.engine.pair_hidden(st, torch.arange(off, off + c1 - c0, device=st["pair_index"].device, dtype=torch.int32))
              for c0, c1, st, off in self["pending"]]
        h = hs[0] if len(hs) == 1 else torch.cat(hs)
        self[key] = h
        return h


@HEADS.register_module()
class RelationTransformerHeadV4(nn.Module):
    # What `tokenizers=None` / `device=None` resolve to.  A config dict such as the reference's
    # (configs/psg/baseline_v4_ov.py:58-63) carries neither keyword; a deployment without hub access points
    # these at local tokenizer objects / a device before `build_detector(cfg.model)`.
    default_tokenizers = "auto"
    default_device = "cuda"

    def __init__(self,
                 # relation qformer (V4:24-32)
                 qformer_model_name='Salesforce/instructblip-vicuna-7b',
                 qformer_instruction='Is there a relation between {} and {}?',
                 patch_size=16,
                 qformer_layer_num=2,
                 qformer_feature_size=768,
                 sampled_qformer_batch_size=32,
                 qformer_neg_over_pos=3,
                 rel_cls_type='binary',
                 rel_cls_loss_weight=50.0,
                 # llm (V4:34-39)
                 llm_model_name='meta-llama/Llama-2-7b-hf',
                 llm_instruction='What are the relations between {} and {}? Assistant: ',
                 llm_truncate_num=-1,
                 llm_feature_size=4096,
                 max_llm_forward_num=4,
                 pair_selector_threshold=0.5,
                 # object and relation (V4:41-44)
                 num_object_classes=133,
                 object_feature_size=256,
                 relation_classes=relation_categories,
                 max_object_num=30,
                 # ---- build-specific, keyword only --------------------------------------------------
                 dtype="bf16",                 # activation/weight dtype of the GPU path: 'bf16' | 'fp16' (both on the
                                               # matrix cores) | 'fp32' (the reference's own precision, exact fp32
                                               # everywhere) | 'fp32s' (fp32 with split-fp16 prompt-pass products)
                                               # | 'mixed' = fp16 GEMM operands with residual_dtype='fp32'
                 residual_dtype=None,          # storage type of the Llama residual stream: None = `dtype` (what HF keeps for
                                               # a model cast to 16 bits) | 'fp32' (never rounded to 16 bits; at 32 layers
                                               # 15 % closer to the fp32 engine for +0.2 % time, tests/test_gpu_llm7b.py)
                 qformer_residual_dtype=None,  # the same for the Q-Former's LayerNorm chain (every LayerNorm then reads an
                                               # fp32 residual and writes fp32 + 16-bit copies).  Built and measured: no
                                               # accuracy gain on the five goldens or the bench scene (two post-LN layers
                                               # of O(1) values), relation query +0.28 ms - so 'mixed' leaves it off
                 device=None,                  # None -> RelationTransformerHeadV4.default_device
                 qformer_vocab_size=30522,
                 llm_config: LlamaConfig | None = None,
                 tokenizers=None,              # None -> default_tokenizers; 'auto': HF tokenizers from the model
                                               # names; 'word': WordTokenizer; or (qformer_tok, llm_tok) objects
                 num_selected=20,              # V4:237
                 max_new_tokens=16,            # V4:308
                 empty_row_policy="uniform",
                 on_parse_error="raise",       # V4:315-316 raises IndexError when no '<s>' was generated
                 implicit_bos=True,            # parse the generation as following an implicit '<s>' (see parse())
                 suppress_eos=False,
                 pair_chunk=12288,             # pairs per Q-Former pass: one pass for up to 110 objects (~6 GB of
                                               # activations at 10 000 pairs in bf16; fewer, larger GEMMs and one prompt
                                               # table per image: 9.5 -> 8.1 ms at 100 objects against chunks of 4096)
                 xattn_variant=None,
                 pair_selector="topk",         # 'topk' (V4:235-237) | 'threshold' (the commented V4:230-234 logic)
                 exclude_diagonal=False,       # the reference never excludes the i == j pairs
                 max_selected=32,              # cap of the threshold selector (one decode batch)
                 prompt_bucket=8,              # Llama prompt grid rounded up to a multiple of this (graph reuse)
                 cls_first=True,               # last Q-Former layer: cls row of every pair -> selection -> rows 1..32
                                               # of the selected pairs only (same results; qformer.forward_pairs_cls)
                 train_dropout=True,           # the gradient path applies the Q-Former dropouts the reference trains with
                                               # (HF defaults 0.1 / 0.1, V4:78-84); False = deterministic (oracle checks)
                 slot_priorities=(0, -1),      # HIP stream priority of submit() slot k = slot_priorities[k % len]: streams
                                               # of different priority never share a hardware queue (see _slot_stream)
                 load_pretrained_llm=True,     # llm_model_name is a LOCAL HuggingFace checkpoint directory: read its
                                               # config.json (unless llm_config is given) and its weights, as the reference's
                                               # from_pretrained does at V4:99-103 (llm_truncate_num layers only).  A hub name
                                               # cannot be resolved here (no network): load_llm_weights() then
                 num_multiclass_triples=100,   # multiclass triples per image (V4:249: k=100), at most 256
                 train_losses_without_grad=False,   # forward() in training mode returns the two losses WITHOUT a graph
                                               # (forward_train); off: it raises, so that an mmdet-style loop cannot sum
                                               # them and silently train nothing in this head
                 llm_rel_scores='constant',    # rel_score of the LLM triples: 'constant' = 1 each (V4:326) | 'likelihood' =
                                               # the decoder's probability of emitting the relation name and stopping
                 num_llm_ranked_triples=0,     # 'likelihood': the N best remaining (pair, class) triples of the selected
                                               # pairs follow the generated ones (at most 4096)
                 llm_decode='greedy',          # 'greedy' = free greedy decode, parse keeps what is a class name (V4:305-321) |
                                               # 'constrained' = every step's arg-max runs over the relation-name trie only:
                                               # each selected pair yields exactly one valid relation in max_depth + 1
                                               # steps, and with 'likelihood' its score comes out of the same launches
                                               # 
                 llm_beam_width=1,             # 1..8, above 1 with 'constrained' + 'likelihood' only: a beam of that width over
                                               # the relation-name trie instead of the greedy walk - every selected pair
                                               # yields up to that many scored relations, in max_depth forwards of
                                               # num_selected x width <= 160 rows on the decode-step kernels.
                                               # An approximation of the pair's best classes; 1 = today's launches
                 llm_weight_quant=None,        # None | 'fp8': the LLM's q/k/v/o/gate/up/down matrices as OCP e4m3fn bytes with one
                                               # fp32 scale per output row (weights.quantize_fp8_rows): decode
                                               # steps of <= 32 rows stream 1 byte per weight.  The model IS the quantised one
                                               # (W' = q s) on every path; an FP8 checkpoint is taken as it is
                                               # 'mxfp4': OCP Microscaling FP4, two E2M1 codes per byte + one exponent byte per 32 k
                                               # + one fp32 scale per row (weights.quantize_mxfp4_rows): 4.25 bits
                                               # per weight in those steps, W' = fp4(q) 2^(e - 127) s likewise
                                               # 'int4g': group-wise INT4 as GPTQ / AWQ checkpoints hold it - 4-bit codes, one fp16
                                               # scale and one 4-bit zero point per 128 weights of a row
                                               # (weights.quantize_int4_groups): 4.25 bits per weight in those steps,
                                               # W' = gs (q - gz); a GPTQ / AWQ checkpoint directory is taken as it is
                 llm_quantize_lm_head=False,   # quantised: the lm_head as well (never the embedding, norms, language_projection)
                 llm_weight_resident='all',    # 'all' | 'quantised': what a quantised LLM keeps in HBM.  'all': W' in
                                               # the engine's dtype beside the bytes (+ the fp16 image of the fp32s prompt
                                               # pass).  'quantised': the bytes, exponents and row scales ONLY - dense operands
                                               # are rebuilt into a scratch buffer right before each product of more than 32
                                               # rows (psg_expand_w8 / _w4), bit for bit the ones 'all' stores; inference only
                 llm_batch_weight_stream='dense',   # 'dense' | 'quantised': what forward_batch's decode steps of 33..160 rows
                                               # read of a quantised LLM.  'dense': W' (today's launches).
                                               # 'quantised': the bytes / nibbles, on psg_batch_gemm_q.hip - 1 / 0.53 bytes per
                                               # weight, and no expansion per step with llm_weight_resident='quantised'
                 llm_batch_split_gemm='library',    # 'library' | 'own': what forward_batch's decode steps of 33..160 rows run
                                               # over the UNQUANTISED matrices of an fp32s head.  'library':
                                               # the SGEMM / the stacked-plane fp16 product (today's launches).  'own':
                                               # psg_batch_gemm_s.hip - two fp16 products over an fp16-valued weight, three
                                               # over the prompt pass's split image of a generic one (4 bytes per weight)
                 llm_bf16_value_stream=False,  # True: an fp32s head whose LLM matrices are bf16 VALUES (a bf16 checkpoint -
                                               # Mistral-7B, Llama-3 - upcast on load; verified per tensor) streams bf16
                                               # copies in the decode steps of <= 32 rows (psg_split_gemm_wb16: 2 bytes per
                                               # weight, three exact bf16 products).  A model whose matrices are not
                                               # bf16 values runs exactly as with False (`llm_engine.bf16_stream_active`)
                 llm_bf16_value_resident=False,  # True (with llm_bf16_value_stream=True): every decoder matrix MUST be a bf16
                                               # value and is held as its bf16 copy ONLY, a bf16-valued lm_head too - 2 bytes
                                               # per weight instead of 12, no fp32 tensor and no split image; every product
                                               # runs on three bf16 planes of the fp32 rows against that copy, the decode
                                               # steps of 33..160 rows on psg_batch_gemm_b3.hip.  Inference only
                 train_precision=None,         # None | 'bf16': the gradient path in the model torch.autocast(bfloat16) gives the
                                               # reference - bf16 activations and products on fp32 masters, with
                                               # any `dtype`; None: the fp32 path of an fp32 head, a 16-bit head does not train
                 **kwargs):
        super().__init__()
        if train_precision not in (None, "bf16"):
            raise PsgHipError(f"train_precision must be None or 'bf16', got {train_precision!r} (fp16 training is not "
                              "offered: 'If use fp16, the loss will be nan', V4)")
        self.train_precision = train_precision
        self._train_llm_copy = None
        if llm_weight_quant not in (None, "fp8", "mxfp4", "int4g"):
            raise PsgHipError(f"llm_weight_quant must be None, 'fp8', 'mxfp4' or 'int4g', got {llm_weight_quant!r}" +
                              (" (group-wise INT4 is spelled 'int4g')" if llm_weight_quant == "int4" else ""))
        if llm_weight_quant is not None and "binary" not in rel_cls_type:
            raise PsgHipError(f"llm_weight_quant={llm_weight_quant!r} quantises the LLM; rel_cls_type={rel_cls_type!r} has no "
                              "LLM stage")
        if llm_weight_resident not in ("all", "quantised"):
            raise PsgHipError(f"llm_weight_resident must be 'all' or 'quantised', got {llm_weight_resident!r}")
        if llm_weight_resident == "quantised" and "binary" not in rel_cls_type:
            raise PsgHipError(f"llm_weight_resident='quantised' is about the LLM's weights; rel_cls_type={rel_cls_type!r} has no "
                              "LLM stage")
        self.llm_weight_resident = llm_weight_resident
        if llm_batch_weight_stream not in ("dense", "quantised"):
            raise PsgHipError(f"llm_batch_weight_stream must be 'dense' or 'quantised', got {llm_batch_weight_stream!r}")
        if llm_batch_weight_stream == "quantised" and "binary" not in rel_cls_type:
            raise PsgHipError(f"llm_batch_weight_stream='quantised' is about the LLM's weights; rel_cls_type={rel_cls_type!r} "
                              "has no LLM stage")
        self.llm_batch_weight_stream = llm_batch_weight_stream
        if llm_batch_split_gemm not in ("library", "own"):
            raise PsgHipError(f"llm_batch_split_gemm must be 'library' or 'own', got {llm_batch_split_gemm!r}")
        if llm_batch_split_gemm == "own" and "binary" not in rel_cls_type:
            raise PsgHipError(f"llm_batch_split_gemm='own' is about the LLM's decode steps; rel_cls_type={rel_cls_type!r} has "
                              "no LLM stage")
        if llm_batch_split_gemm == "own" and dtype != "fp32s":
            raise PsgHipError(f"llm_batch_split_gemm='own' runs the fp32s batched decode on split-fp16 products; dtype={dtype!r}: "
                              "the 16-bit modes already run psg_batch_gemm there, and the exact 'fp32' mode keeps its exact SGEMM "
                              "- use dtype='fp32s' or llm_batch_split_gemm='library'")
        self.llm_batch_split_gemm = llm_batch_split_gemm
        if not isinstance(llm_bf16_value_stream, bool):
            raise PsgHipError(f"llm_bf16_value_stream must be True or False, got {llm_bf16_value_stream!r}")
        if llm_bf16_value_stream and "binary" not in rel_cls_type:
            raise PsgHipError(f"llm_bf16_value_stream=True is about the LLM's decode steps; rel_cls_type={rel_cls_type!r} has "
                              "no LLM stage")
        if llm_bf16_value_stream and dtype != "fp32s":
            raise PsgHipError(f"llm_bf16_value_stream=True streams bf16-valued weights under the fp32s decode steps; "
                              f"dtype={dtype!r}: the 16-bit modes already stream 2 bytes per weight, and the exact 'fp32' mode "
                              "keeps its fp32 products - use dtype='fp32s' or llm_bf16_value_stream=False")
        if llm_bf16_value_stream and llm_weight_quant is not None:
            raise PsgHipError(f"llm_bf16_value_stream=True streams the UNQUANTISED bf16 values of the LLM; with "
                              f"llm_weight_quant={llm_weight_quant!r} the decode steps stream the quantised bytes - set one of "
                              "the two")
        self.llm_bf16_value_stream = llm_bf16_value_stream
        if not isinstance(llm_bf16_value_resident, bool):
            raise PsgHipError(f"llm_bf16_value_resident must be True or False, got {llm_bf16_value_resident!r}")
        if llm_bf16_value_resident and not llm_bf16_value_stream:
            raise PsgHipError("llm_bf16_value_resident=True keeps the bf16 copies of llm_bf16_value_stream as the ONLY copy of the "
                              "LLM's matrices: it needs llm_bf16_value_stream=True (an fp32s head with an LLM stage and no "
                              "llm_weight_quant)")
        self.llm_bf16_value_resident = llm_bf16_value_resident
        if llm_quantize_lm_head and llm_weight_quant is None:
            raise PsgHipError("llm_quantize_lm_head=True needs llm_weight_quant='fp8' or 'mxfp4' or 'int4g'")
        # group-wise INT4 has the decode kernels of <= 32 rows only: no expand kernel, no 33..160-row kernel
        if llm_weight_quant == "int4g" and llm_weight_resident == "quantised":
            raise PsgHipError("llm_weight_resident='quantised' is not built for the INT4 format (llm_weight_quant='int4g'): "
                              "there is no expand kernel for it - use llm_weight_resident='all'")
        if llm_weight_quant == "int4g" and llm_batch_weight_stream == "quantised":
            raise PsgHipError("llm_batch_weight_stream='quantised' is not built for the INT4 format (llm_weight_quant='int4g'): "
                              "there is no 33..160-row kernel for it - use llm_batch_weight_stream='dense'")
        self.llm_weight_quant = llm_weight_quant
        self.llm_quantize_lm_head = bool(llm_quantize_lm_head)
        if rel_cls_type not in REL_CLS_TYPES:
            raise ValueError(f"rel_cls_type must be one of {REL_CLS_TYPES} (V4:31, 91-95), got {rel_cls_type!r}")
        if llm_rel_scores not in ("constant", "likelihood"):
            raise PsgHipError(f"llm_rel_scores must be 'constant' or 'likelihood', got {llm_rel_scores!r}")
        self.llm_rel_scores = llm_rel_scores
        self.num_llm_ranked_triples = int(num_llm_ranked_triples)
        if not 0 <= self.num_llm_ranked_triples <= MAX_RANKED_TRIPLES:
            raise PsgHipError(f"num_llm_ranked_triples must be in 0..{MAX_RANKED_TRIPLES}, got {num_llm_ranked_triples}")
        if self.num_llm_ranked_triples > 0 and llm_rel_scores != "likelihood":
            raise PsgHipError("num_llm_ranked_triples > 0 ranks (pair, class) triples by their decoder likelihood: it needs "
                              "llm_rel_scores='likelihood'")
        if llm_rel_scores == "likelihood" and "binary" not in rel_cls_type:
            raise PsgHipError(f"llm_rel_scores='likelihood' scores the LLM triples; rel_cls_type={rel_cls_type!r} has no "
                              "LLM stage")
        if llm_rel_scores == "likelihood" and not implicit_bos:
            raise PsgHipError("llm_rel_scores='likelihood' needs implicit_bos=True: a candidate is what generate emits after "
                              "the prompt, and with implicit_bos=False parse reads nothing from a text without '<s>'")
        if llm_decode not in ("greedy", "constrained"):
            raise PsgHipError(f"llm_decode must be 'greedy' or 'constrained', got {llm_decode!r}")
        if llm_decode == "constrained" and "binary" not in rel_cls_type:
            raise PsgHipError(f"llm_decode='constrained' constrains the LLM's decode; rel_cls_type={rel_cls_type!r} has no LLM "
                              "stage")
        if llm_decode == "constrained" and not implicit_bos:
            raise PsgHipError("llm_decode='constrained' needs implicit_bos=True: a candidate is what generate emits after the "
                              "prompt, and with implicit_bos=False parse reads nothing from a text without '<s>'")
        if llm_decode == "constrained" and suppress_eos:
            raise PsgHipError("llm_decode='constrained' cannot run with suppress_eos=True: a constrained sequence is a relation "
                              "name followed by EOS by definition")
        self.llm_decode = llm_decode
        if isinstance(llm_beam_width, bool) or not isinstance(llm_beam_width, (int, np.integer)) or not 1 <= llm_beam_width <= 8:
            raise PsgHipError(f"llm_beam_width must be an int in 1..8, got {llm_beam_width!r}")
        self.llm_beam_width = int(llm_beam_width)
        if self.llm_beam_width > 1:
            if llm_decode != "constrained":
                raise PsgHipError(f"llm_beam_width={self.llm_beam_width} is a beam over the relation-name trie: it needs "
                                  f"llm_decode='constrained', got {llm_decode!r}")
            if llm_rel_scores != "likelihood":
                raise PsgHipError(f"llm_beam_width={self.llm_beam_width} returns several SCORED relations per pair: it needs "
                                  f"llm_rel_scores='likelihood', got {llm_rel_scores!r}")
            if self.num_llm_ranked_triples > 0:
                raise PsgHipError(f"llm_beam_width={self.llm_beam_width} with num_llm_ranked_triples="
                                  f"{self.num_llm_ranked_triples}: the trie pass is the other way to several scored relations "
                                  "per pair - set one of the two")
            rows = max(int(num_selected), int(max_selected) if pair_selector == "threshold" else 0)
            if rows * self.llm_beam_width > 160:
                raise PsgHipError(f"llm_beam_width={self.llm_beam_width}: {rows} selected pairs x {self.llm_beam_width} "
                                  f"hypotheses = {rows * self.llm_beam_width} rows exceed the 160 rows of the decode-step "
                                  "kernels (num_selected, or max_selected under pair_selector='threshold')")
        # 'binary': existence head -> top-20 pairs -> LLM decode (V4:206-209, 235-237).  'multiclass' in the type: one
        # sigmoid score per (pair, relation class) from multiclass_rel_cls_pred, the diagonal zeroed, the top
        # `num_multiclass_triples` (pair, class) scores returned behind the LLM triples (V4:238-257, 355-356)
        self.has_binary = "binary" in rel_cls_type
        self.has_multiclass = "multiclass" in rel_cls_type
        self.num_multiclass_triples = int(num_multiclass_triples)
        if not 1 <= self.num_multiclass_triples <= 256:
            raise PsgHipError(f"num_multiclass_triples must be in 1..256, got {num_multiclass_triples}")
        if self.has_multiclass and not 1 <= len(relation_classes) <= 128:
            raise PsgHipError(f"the multiclass head runs up to 128 relation classes, got {len(relation_classes)}")
        self.qformer_instruction = qformer_instruction
        self.sampled_qformer_batch_size = int(sampled_qformer_batch_size)
        self.qformer_neg_over_pos = int(qformer_neg_over_pos)
        self.rel_cls_loss_weight = float(rel_cls_loss_weight)
        self.llm_instruction = llm_instruction
        self.rel_cls_type = rel_cls_type
        self.llm_truncate_num = llm_truncate_num
        self.pair_selector_threshold = pair_selector_threshold
        self.relation_classes = list(relation_classes)
        self.num_relation_classes = len(self.relation_classes)
        self.num_object_classes = num_object_classes
        self.max_object_num = max_object_num
        self.on_parse_error = on_parse_error
        self.implicit_bos = bool(implicit_bos)
        self.suppress_eos = suppress_eos
        self.pair_chunk = int(pair_chunk)
        self.xattn_variant = xattn_variant
        assert pair_selector in ("topk", "threshold")
        self.pair_selector = pair_selector
        self.exclude_diagonal = bool(exclude_diagonal)
        self.max_llm_forward_num = max_llm_forward_num
        self.max_selected = int(max_selected)
        self.prompt_bucket = int(prompt_bucket)
        self.cls_first = bool(cls_first)
        self.train_losses_without_grad = bool(train_losses_without_grad)
        self.train_dropout = bool(train_dropout)
        self.act_dtype = _DTYPES[dtype]
        # 'fp32s' = the fp32 mode with the prompt pass's projections as split-fp16 products on the 16-bit matrix cores
        # (x.w = xh.wh + xh.wl + xl.wh, fp32 accumulation, ~7e-7 per product instead of fp32's 6e-8; llm.py, psg_split.hip):
        # everything else - Q-Former, decode steps, KV cache, attention - is the fp32 mode's own exact-fp32 arithmetic
        self.prefill_split = dtype == "fp32s"
        if residual_dtype is None and dtype in ("mixed", "mixed_q32"):
            residual_dtype = "fp32"
        if qformer_residual_dtype is None and dtype == "mixed_q32":    # 'mixed' + the Q-Former's residual chain in fp32
            qformer_residual_dtype = "fp32"
        self.resid_dtype = self.act_dtype if residual_dtype is None else _DTYPES[residual_dtype]
        if self.resid_dtype not in (self.act_dtype, torch.float32):
            raise PsgHipError(f"residual_dtype must be the activation dtype or 'fp32', got {residual_dtype!r}")
        self.q_resid_dtype = self.act_dtype if qformer_residual_dtype is None else _DTYPES[qformer_residual_dtype]
        if self.q_resid_dtype not in (self.act_dtype, torch.float32):
            raise PsgHipError(f"qformer_residual_dtype must be the activation dtype or 'fp32', got {qformer_residual_dtype!r}")
        self.device = torch.device(self.default_device if device is None else device)
        if tokenizers is None:
            tokenizers = self.default_tokenizers
        self.llm_model_name = llm_model_name
        pretrained_dir = bool(load_pretrained_llm) and is_hf_checkpoint_dir(llm_model_name)
        if llm_batch_weight_stream == "quantised" and llm_weight_quant is None and not pretrained_dir:
            # (a checkpoint directory may hold a quantised model: the engine refuses it at load time if it does not)
            raise PsgHipError("llm_batch_weight_stream='quantised' streams a quantised LLM's bytes: set llm_weight_quant='fp8' / "
                              "'mxfp4' or load an FP8 / MXFP4 checkpoint directory ('int4g' has no such kernel)")
        if llm_config is not None:
            llm = llm_config
        elif pretrained_dir:
            # the architecture from_pretrained would build; grouped-query checkpoints (Mistral-7B, ...) included
            llm = read_hf_llama_config(llm_model_name, grouped_query=True)
        else:
            llm = LlamaConfig(hidden=llm_feature_size, heads=llm_feature_size // 128)
        if llm.hidden != llm_feature_size:
            raise PsgHipError(f"llm_feature_size={llm_feature_size} must match the LLM's hidden size {llm.hidden} "
                              "(language_projection maps onto its embedding rows, V4:97-98)")
        self.cfg = PSGConfig(
            qformer=QFormerConfig(hidden=qformer_feature_size, layers=qformer_layer_num, vocab=qformer_vocab_size,
                                  enc_hidden=object_feature_size),
            llm=llm, patch_size=patch_size, feat_channels=object_feature_size, max_object_num=max_object_num,
            max_new_tokens=max_new_tokens, num_selected=num_selected, empty_row_policy=empty_row_policy,
            rel_cls_type=rel_cls_type, num_relation_classes=self.num_relation_classes)
        # parameters under the reference's names (fp32 masters; the engines keep packed copies)
        for key, shape in head_shapes(self.cfg).items():
            _set_nested(self, key, torch.zeros(shape, dtype=torch.float32, device=self.device))
        # Trainable from construction in an fp32 head (the gradient path is fp32), whatever the training flag says: an
        # mmdet-style flow wraps the model in DistributedDataParallel BEFORE runner.train() calls model.train(), and DDP
        # registers its reducer hooks for the parameters that require a gradient at that moment.  A caller's own
        # freezes (requires_grad_(False) on part of the head) are never touched again.
        # train_precision='bf16' trains the fp32 masters of a head of any dtype: the same argument applies.
        for p_ in self.parameters():
            p_.requires_grad_(self.act_dtype == torch.float32 or self.train_precision is not None)
        self._engine_version = None
        self._llm_weights = None
        self._rq_engine = None
        self._llm_engine = None
        self._prompt_store = {k: dict(names=[], index={}, ids=np.zeros((0, 0, 0), np.int32), lens=np.zeros((0, 0), np.int32))
                              for k in ("q", "l")}
        self._table_cache = {}
        # tokenizers (V4:85-86, 104-105)
        if tokenizers == "word":
            self.relation_qformer_tokenizer = WordTokenizer("bert")
            self.llm_tokenizer = WordTokenizer("llama")
        elif tokenizers == "auto":
            try:
                from transformers import AutoTokenizer
                self.relation_qformer_tokenizer = AutoTokenizer.from_pretrained(qformer_model_name,
                                                                                subfolder="qformer_tokenizer")
                self.llm_tokenizer = AutoTokenizer.from_pretrained(llm_model_name)
            except Exception as e:  # noqa: BLE001
                raise PsgHipError(
                    f"cannot load the HF tokenizers for {qformer_model_name!r} / {llm_model_name!r} ({e}); pass local "
                    "paths, tokenizer objects via tokenizers=(qformer_tok, llm_tok), or tokenizers='word'") from e
        else:
            self.relation_qformer_tokenizer, self.llm_tokenizer = tokenizers
        self.llm_tokenizer.pad_token = self.llm_tokenizer.unk_token        # V4:105
        self._rel_trie = self._rel_trie_tok = None
        if self.llm_rel_scores == "likelihood" or self.llm_decode == "constrained":
            self.relation_trie()                                            # checks the candidates now: fails early
        self.last = {}
        self._gather_cache = {}
        # Two slots whose streams share a hardware queue run one after the other (67.8 instead of 57 ms per image), and
        # which of its GPU_MAX_HW_QUEUES queues HIP binds a stream to depends on the order in which every stream of the
        # process is first used.  Streams of different PRIORITY never share a queue (HIP keeps one queue pool per
        # priority), so odd slots are high-priority streams; the first two are created and first used here.
        self._slot_streams = {}
        self.slot_priorities = tuple(int(p) for p in slot_priorities)
        if torch.cuda.is_available() and self.device.type == "cuda":
            for slot in (0, 1):
                self._slot_stream(slot)
        self._decode_done = None
        self._decode_done_slot = None
        self._slot_pending = {}
        self._front_done = None
        # submit(): image k+1's decode steps wait for image k's (its relation query and prompt pass do not).  Measured A/B
        # at BASELINE C3, two slots: serialised 67.4 ms per image = no gain over one image at a time; free-running 56.6.
        # What overlaps is decode beside decode: the latency-bound row kernels and the fixed start / tail of every
        # weight-streaming launch of one image run under the other image's streaming - not prompt pass beside decode
        # (a decode launch holds every CU's LDS; a library GEMM workgroup cannot move in next to it)
        self.serialize_decodes = False
        self._proj_stale = False
        self.train(False)                                                   # eval by default, as init_detector leaves it
        if pretrained_dir and hf_checkpoint_has_weights(llm_model_name):     # (config + tokenizer only: load_llm_weights() later)
            # V4:99-103: the LLM comes from `llm_model_name`, not from the head's checkpoint (part_checkpoint_hook.py:96-116
            # drops language_model.*).  language_projection is loaded later: the engine's copy follows it (_proj_stale)
            n = self.cfg.llm.layers if self.llm_truncate_num <= 0 else self.llm_truncate_num
            self.load_llm_weights(read_hf_llama_weights(llm_model_name, n_layers=n))
            self._proj_stale = True

    # ---- weights ---------------------------------------------------------------------------------
    def load_weights(self, weights: dict):
        """Loads head (and, if present, `language_model.*`) tensors given under the reference names."""
        llm = {k: v for k, v in weights.items() if k.startswith("language_model.")}
        own = dict(self.named_parameters())
        for k, v in weights.items():
            if k in own:
                own[k].data.copy_(v.to(torch.float32))
        if llm:
            self.load_llm_weights(llm)
        self._rq_engine = None
        return self

    def load_state_dict(self, state_dict, strict=False, **kw):  # reference checkpoints are partial
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        """Runs in every loading flow: `head.load_state_dict`, a parent's `load_state_dict` (the detector's,
        keys `relation_head.*`) and mmcv's `load_checkpoint`, which all recurse through this method.  The packed
        engine copies are dropped (rebuilt lazily from the freshly loaded fp32 masters) and `language_model.*`
        tensors - absent from reference checkpoints (part_checkpoint_hook.py:96-116), present in full ones - are
        routed to the decode engine instead of being reported as unexpected."""
        lm = prefix + "language_model."
        llm = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(lm)}
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)
        unexpected_keys[:] = [k for k in unexpected_keys if not k.startswith(lm)]
        self._rq_engine = None
        # this hook runs BEFORE torch recurses into the children, i.e. before language_projection.* of this
        # checkpoint is loaded: the decode engine's packed copy of the projection is refreshed at its next use
        self._proj_stale = True
        if llm:
            self.load_llm_weights(llm)

    def load_llm_weights(self, weights: dict):
        """`language_model.*` tensors (HF LlamaForCausalLM names); V4:99-103."""
        need = llm_shapes(self.cfg)
        n_layers = self.cfg.llm.layers if self.llm_truncate_num <= 0 else self.llm_truncate_num
        missing = [k for k in need if k not in weights and
                   not (".layers." in k and int(k.split(".layers.")[1].split(".")[0]) >= n_layers)]
        if missing:
            raise PsgHipError(f"LLM weights missing {len(missing)} tensors, e.g. {missing[:3]}")
        def stored(k):                                  # an MXFP4 / INT4 matrix [N, K] comes as two codes per byte: [N, K / 2]
            return (need[k][0], need[k][1] // 2) if k + "_bexp" in weights or k + "_gscale" in weights else need[k]
        wrong = [(k, tuple(weights[k].shape), stored(k)) for k in need if k in weights and tuple(weights[k].shape) != stored(k)]
        if wrong:                                       # e.g. a grouped-query checkpoint under a multi-head config
            raise PsgHipError(f"LLM weights of the wrong shape ({len(wrong)}), e.g. {wrong[:2]} "
                              f"({self.cfg.llm.heads} query / {self.cfg.llm.n_kv_heads} key-value heads)")
        if any(k.endswith("_gscale") for k in weights) and (self.llm_weight_resident == "quantised"
                                                            or self.llm_batch_weight_stream == "quantised"):
            opt = "llm_weight_resident" if self.llm_weight_resident == "quantised" else "llm_batch_weight_stream"
            raise PsgHipError(f"{opt}='quantised' is not built for the INT4 format (a GPTQ / AWQ checkpoint): there is no "
                              "expand kernel and no 33..160-row kernel for it")
        if self.llm_weight_resident == "quantised":
            # the dense model never reaches the device: a matrix is quantised where it lives, uploaded and dropped when the
            # engine asks for it (peak = the final footprint + the pieces of one matrix in flight)
            from .weights import LazyQuantWeights
            quant = llm_quant_keys(n_layers, self.llm_quantize_lm_head) if self.llm_weight_quant is not None else []
            w = LazyQuantWeights(weights, quant, self.llm_weight_quant, self.device)
        else:
            w = self.quantize_llm_weights(weights)
        w["language_projection.weight"] = self.language_projection.weight.data
        w["language_projection.bias"] = self.language_projection.bias.data
        self._llm_engine = LlamaDecodeEngine(w, self.cfg, self.device, self.act_dtype, n_layers=n_layers,
                                             resid_dtype=self.resid_dtype, prefill_split=self.prefill_split,
                                             resident=self.llm_weight_resident,
                                             batch_quant_stream=self.llm_batch_weight_stream == "quantised",
                                             batch_split_gemm=self.llm_batch_split_gemm == "own",
                                             bf16_value_stream=self.llm_bf16_value_stream,
                                             bf16_value_resident=self.llm_bf16_value_resident)
        return self

    def quantize_llm_weights(self, weights: dict) -> dict:
        """What `load_llm_weights` hands the decode engine: with llm_weight_quant='fp8' every q/k/v/o/gate/up/down matrix
        of the kept layers (+ the lm_head with llm_quantize_lm_head) as (e4m3fn bytes under its name, fp32 row scales
        under name + '_scale'), with 'mxfp4' as (fp4 nibbles, name + '_bexp', name + '_scale'), with 'int4g' as (4-bit codes,
        name + '_gscale', name + '_gzero'); matrices that already come quantised are kept.  Otherwise a plain copy of the dict."""
        if self.llm_weight_quant is None:
            return dict(weights)
        from .weights import quantize_llm_weights
        n_layers = self.cfg.llm.layers if self.llm_truncate_num <= 0 else self.llm_truncate_num
        return quantize_llm_weights(weights, n_layers, self.llm_quantize_lm_head, self.llm_weight_quant)

    def _param_version(self) -> int:
        """Sum of the parameters' in-place version counters: every optimizer step (and any other in-place update of a
        parameter) moves it, so packed engine copies older than the masters are detected without a hook."""
        return sum(int(p._version) for p in self.parameters())

    @property
    def rq_engine(self) -> RelationQueryEngine:
        # training mode: optimizer steps move the masters under the packed copies (eval-mode flows invalidate
        # explicitly - load_*, train(False) - and skip the 70-tensor walk on the inference path)
        ver = self._param_version() if self.training else self._engine_version
        if self._rq_engine is not None and ver != self._engine_version:
            self._rq_engine = None
        if self._rq_engine is None:
            w = {k: v.data for k, v in self.named_parameters()}
            self._rq_engine = RelationQueryEngine(w, self.cfg, self.device, self.act_dtype, self.xattn_variant,
                                                  resid_dtype=self.q_resid_dtype, split=self.prefill_split)
            self._engine_version = ver
            self._proj_stale = True              # language_projection may have been (re)loaded: see llm_engine
        return self._rq_engine

    @property
    def llm_engine(self) -> LlamaDecodeEngine:
        if self._llm_engine is None:
            raise PsgHipError("the LLM weights are not loaded: reference checkpoints do not contain "
                              "`language_model.*` (part_checkpoint_hook.py:96-116); call load_llm_weights()")
        if self.training:
            ver = self._param_version()
            if ver != getattr(self, "_proj_version", None):  # an optimizer step moved language_projection
                self._proj_stale, self._proj_version = True, ver
        if getattr(self, "_proj_stale", False):               # language_projection was (re)loaded after the engine was built
            self._llm_engine.set_projection(self.language_projection.weight.data, self.language_projection.bias.data)
            self._proj_stale = False
        return self._llm_engine

    # ---- prompts (V4:146-152, 260-266) ---------------------------------------------------------------
    def _prompt_table(self, kind: str, names):
        """Token ids of the prompt of every ordered pair of the UNIQUE names of this image.  A prompt is tokenised once
        per pair of names, ever: the head keeps one padded store per tokenizer over all names seen so far
        ([G, G, Tcap] ids with -1 behind the valid tokens, [G, G] lengths), and an image's table is a slice of it -
        a new image costs a few array operations on the host, not a tokenizer call or a Python loop per pair.
        Returns (uniq index per object, U, ids [U*U, Tcap] int32 (-1 padded, valid tokens first), lens [U*U] int32)."""
        st = self._prompt_store[kind]
        uniq = sorted(set(names))
        new = [n for n in uniq if n not in st["index"]]
        if new:
            old = list(st["names"])
            todo = [(a, b) for a in old + new for b in new] + [(a, b) for a in new for b in old]
            if kind == "q":
                tok, tmpl = self.relation_qformer_tokenizer, self.qformer_instruction
            else:
                tok, tmpl = self.llm_tokenizer, self.llm_instruction
                tok.padding_side = "left"                                                     # V4:262
            enc = tok([tmpl.format(a, b) for a, b in todo], return_tensors="pt", padding=True,
                      return_attention_mask=True)
            ids, mask = np.asarray(enc["input_ids"]), np.asarray(enc["attention_mask"]).astype(bool)
            lens = mask.sum(1).astype(np.int32)
            for n in new:
                st["index"][n] = len(st["names"])
                st["names"].append(n)
            G, cap = len(st["names"]), max(int(lens.max()), st["ids"].shape[2])
            gi = np.full((G, G, cap), -1, dtype=np.int32)
            gl = np.zeros((G, G), dtype=np.int32)
            g0 = st["ids"].shape[0]
            gi[:g0, :g0, :st["ids"].shape[2]] = st["ids"]
            gl[:g0, :g0] = st["lens"]
            ia = np.array([st["index"][a] for a, _ in todo]), np.array([st["index"][b] for _, b in todo])
            order = np.argsort(~mask, axis=1, kind="stable")                               # valid tokens first, original order
            comp = np.take_along_axis(ids, order, axis=1).astype(np.int32)
            comp[np.arange(ids.shape[1])[None, :] >= lens[:, None]] = -1
            gi[ia[0], ia[1], :ids.shape[1]] = comp
            gl[ia[0], ia[1]] = lens
            st["ids"], st["lens"] = gi, gl
        uidx = [uniq.index(n) for n in names]
        g = np.array([st["index"][n] for n in uniq])
        U = len(uniq)
        ids = st["ids"][np.ix_(g, g)].reshape(U * U, -1)
        lens = st["lens"][np.ix_(g, g)].reshape(U * U)
        return uidx, U, ids, lens

    def warm_prompts(self, names=None):
        """Tokenises the prompts of every ordered pair of `names` (default: all 133 object classes, 17 689 pairs per
        tokenizer) into the prompt stores in two tokenizer calls, so that no image ever waits for a tokenizer.  A
        deployment calls this once after construction (tools/infer.py does); without it the stores fill as classes
        appear."""
        names = sorted(set(object_categories if names is None else names))
        for kind in ("q", "l"):
            self._prompt_table(kind, names)

    # ---- forward ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def _unpack(self, inputs):
        feat = inputs['mask_features']
        meta = inputs['img_metas'][0]
        assert feat.shape[0] == 1, 'only support batch size 1 for now.'                    # V4:112
        if not feat.is_cuda:
            raise PsgHipError("mask_features must live in HBM; this head has no CPU path")
        info = inputs['object_info'][0]
        ids = list(info['object_id_list'][:self.max_object_num])                            # V4:136
        if ids and torch.is_tensor(ids[0]) and ids[0].is_cuda:
            ids = torch.stack([t.reshape(()) for t in ids]).cpu().tolist()                  # one copy, not N synchronisations
        obj_ids = [int(x) for x in ids]
        names = [object_categories[i % INSTANCE_OFFSET] for i in obj_ids]                  # V4:138-139
        return feat, meta, info, obj_ids, names

    def forward(self, inputs, is_generation=None):
        if self.training:
            if (self.act_dtype == torch.float32 or self.train_precision is not None) and torch.is_grad_enabled():
                return self.forward_train_grad(inputs)            # the losses with their gradient graph (V4:345-351)
            if not self.train_losses_without_grad:
                raise NotImplementedError(
                    "RelationTransformerHeadV4.forward in training mode: the gradient path runs in fp32 with autograd "
                    "enabled (dtype='fp32'); in a 16-bit head or under no_grad only the loss VALUES are available, and a "
                    "training loop summing them would train nothing.  Call forward_train(inputs) for the values, or "
                    "construct the head with train_losses_without_grad=True to get them from forward().")
            return self.forward_train(inputs)
        feat, meta, info, obj_ids, names = self._unpack(inputs)
        N = len(obj_ids)
        if N == 0:
            return dict(rel_pred=[], rel_score=[])
        rq = self.run_relation_query(feat, meta, obj_ids, names, info["pan_results"])
        if is_generation is None:
            is_generation = True
        is_generation = is_generation and self.has_binary        # 'multiclass' alone: no pair selector, no decode
        out = self.decode_selected(rq, names) if is_generation else dict(tokens=None)
        if self.has_multiclass:                               # behind the tokens' copy: the stream has drained
            out["mc_host"] = rq["mc_topk"].cpu().numpy()
        rq.update(out)                                        # keeps a lazy rq lazy (`hidden` on demand)
        self.last = rq
        rel_pred, rel_score = self._parse_out(out, N) if is_generation else ([], [])
        mc_pred, mc_score = self.parse_multiclass(out.get("mc_host"), N)
        return dict(rel_pred=rel_pred + mc_pred, rel_score=rel_score + mc_score)   # V4:355-356

    # ---- two images in flight -------------------------------------------------------------------------------------------
    def submit(self, inputs, slot=0):
        """`forward` without its final host synchronisation: everything is enqueued on the slot's own HIP stream and a
        handle is returned; `handle.result()` waits for that stream only, copies the token ids back and parses them
        (same dict as `forward`).  With two slots the caller keeps two images in flight:

            pending = head.submit(image_k1, slot=(k + 1) % 2)      # relation query + prompt pass: matrix-core bound
            result_k = previous.result()                           # image k's decode steps: HBM bound, already running

        Two images' kernels then interleave on the GPU: 1.19x images per second on one MI355X at BASELINE C3 (56.6 against
        67.4 ms per image; three in flight: 60.6), every result identical to `forward`'s.  The gain is decode beside
        decode - an image's latency-bound row kernels (22 us per layer) and the fixed start / tail of its weight-streaming
        launches run under the other image's streaming (A/B: `serialize_decodes`).  The reference handles one image
        per call (V4:112); this is the same call, issued one image ahead.  A slot owns its decode graphs (KV caches,
        static buffers; `forward` has its own) and must not be re-submitted before its pending result was taken."""
        if self.training:
            raise PsgHipError("submit: inference only")
        live = self._slot_pending.get(slot)
        live = live() if live is not None else None
        if live is not None and not live.taken and live.rq is not None:
            # the slot's decode graphs hand out their static token buffers at result(): a second image on the slot would
            # silently return ITS tokens for the first handle
            raise PsgHipError(f"submit: slot {slot} still holds an image whose result() was not taken")
        st = self._slot_stream(slot)
        st.wait_stream(torch.cuda.current_stream(self.device))          # the inputs were produced on the caller's stream
        with torch.cuda.stream(st):
            feat, meta, info, obj_ids, names = self._unpack(inputs)
            N = len(obj_ids)
            if N == 0:
                return _Pending(self, st, None, None, 0, slot=slot)
            # the caller may drop its tensors as soon as this returns (a detector's mask_features are a temporary): the
            # caching allocator must not hand their blocks out again before the slot stream has read them
            for t in (feat, info["pan_results"], *[x for x in info['object_id_list'] if torch.is_tensor(x)]):
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(st)
            # The front halves (relation query + prompt pass: the only part with LIBRARY GEMMs) of consecutive images are
            # ordered by an event - free in the steady state, where image k's front half ended long before image k+1 is
            # submitted -, so that two library GEMMs never run side by side on two streams: hipBLASLt kernels with a
            # workspace (stream-K / split-K, picked at 40-80 rows) were seen to dead-lock the GPU that way
            # (tools/inflight_stress.py batch).  What overlaps is image k's decode steps - own kernels only - with
            # image k+1's front half and decode.
            self._wait_front(st)
            rq = self.run_relation_query(feat, meta, obj_ids, names, info["pan_results"])
            out = self._enqueue_decode(st, rq, names, slot, defer=True) if self.has_binary else dict(tokens=None)
        pend = _Pending(self, st, rq, out, N, inputs=inputs, slot=slot)
        self._slot_pending[slot] = weakref.ref(pend)                   # (a dropped handle frees its slot)
        return pend

    def _slot_stream(self, slot):
        st = self._slot_streams.get(slot)
        if st is None:
            st = self._slot_streams[slot] = torch.cuda.Stream(
                device=self.device, priority=self.slot_priorities[slot % len(self.slot_priorities)])
            with torch.cuda.stream(st):
                torch.zeros(1, device=self.device)             # first use: binds the stream to its hardware queue now
        return st

    def _wait_front(self, st):
        """Orders the library-GEMM phases of consecutive images (see `submit`); with more than 32 decode rows the decode
        steps hold library GEMMs too and nothing may overlap."""
        if self._front_done is not None:
            st.wait_event(self._front_done)
        rows = max(self.cfg.num_selected, self.max_selected if self.pair_selector == "threshold" else 0)
        rows *= self.llm_beam_width                             # a beam's levels are forwards of pairs x width rows
        if self._decode_done is not None and (rows > 32 or self.cfg.num_selected > 32 or (
                self.pair_selector == "threshold" and self.max_selected > 32) or not self.llm_engine.use_skinny
                or self.llm_engine.decode_uses_library(rows)):
            st.wait_event(self._decode_done)

    def _enqueue_decode(self, st, rq, names, slot, selected=None, pair_features=None, defer=False):
        """The decode of one image on slot stream `st` (the caller is inside `torch.cuda.stream(st)` and has called
        `_wait_front`): prompt pass, event, decode steps; no host wait with `defer` (natural EOS: the chunks behind the
        first are replayed by `out["_finish"]`)."""
        prev, front_done, gated = self._decode_done, torch.cuda.Event(), [False]

        def gate():                                             # between the prompt pass and the decode steps
            front_done.record(st)
            gated[0] = True
            if prev is not None and self.serialize_decodes:         # A/B switch: decode steps of two images never overlap
                st.wait_event(prev)
        # graph slot 0 belongs to `forward` (the caller's stream): a pending submit never shares its KV caches
        out = self.decode_selected(rq, names, selected=selected, pair_features=pair_features, to_host=False,
                                   slot=slot + 1, gate=gate, defer=defer)
        if not gated[0]:                                        # eager run, or every pair ended inside the first graph
            front_done.record(st)
        self._front_done = front_done
        self._decode_done = torch.cuda.Event()
        self._decode_done.record(st)
        self._decode_done_slot = slot
        return out

    def decode_concurrent(self, items):
        """The decodes of several images side by side: items[p] = dict(rq, names, selected, pair_features) runs on slot
        stream p like a `submit` (its prompt pass ordered behind the previous item's, its decode steps beside the
        others'), and the caller's stream waits for all of them.  Returns the `decode_selected` dicts (device tensors).
        Used by the pair-sharded pipeline when a rank owns more than one image of a step (dist.step_gen)."""
        cur = torch.cuda.current_stream(self.device)
        outs = []
        for p, it in enumerate(items):
            st = self._slot_stream(p)
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                self._wait_front(st)
                out = self._enqueue_decode(st, it["rq"], it["names"], p, selected=it.get("selected"),
                                           pair_features=it.get("pair_features"))
            for t in out.values():
                if isinstance(t, torch.Tensor):
                    t.record_stream(cur)                        # allocated on the slot stream, consumed on the caller's
            outs.append(out)
        for p in range(len(items)):
            cur.wait_stream(self._slot_stream(p))
        return outs

    # ---- training branch: forward arithmetic of the losses -------------------------------------
    def qformer_sampler(self, relation_target):
        """V4:437-461: positive pairs + up to qformer_neg_over_pos x as many negatives (torch's CPU generator)."""
        t = relation_target.reshape(-1, self.num_relation_classes).sum(1)
        pos = torch.nonzero(t, as_tuple=False)[:, 0]
        neg = torch.nonzero(t == 0, as_tuple=False)[:, 0]
        pn, nn_, bs, k = pos.shape[0], neg.shape[0], self.sampled_qformer_batch_size, self.qformer_neg_over_pos
        if pn < bs:
            sp = pos
            sn = neg[torch.randint(0, nn_, (min(bs - pn, pn * k),))]
        else:
            sp = pos[torch.randint(0, pn, (bs // (k + 1),))]
            sn = neg[torch.randint(0, nn_, (bs * k // (k + 1),))]
        return torch.cat([sp, sn], dim=0)

    def _train_prepare(self, inputs, sampled=None, selected=None):
        """Host side of the training branch (V4:114-133, 218-228, 260-285, 360-406): relation targets, ground-truth object
        masks on the patch grid (HIP, bit-exact), the sampled pairs and their BERT prompts, the LLM selection with its
        prompt / label token grids.  `sampled` / `selected` replace the random draws (V4:173 `qformer_sampler`,
        V4:222-228 `random.sample`).  Returns a dict shared by the loss-only and the gradient paths."""
        import random
        if self.llm_weight_resident == "quantised" and self.has_binary:
            raise PsgHipError("llm_weight_resident='quantised' is an inference mode: the training forward would keep views of "
                              "an expansion scratch that the next product overwrites - build the head with "
                              "llm_weight_resident='all' to train")
        if self.llm_bf16_value_resident and self.has_binary:
            raise PsgHipError("llm_bf16_value_resident=True is an inference mode: the training forward reads the fp32 tensors "
                              "of the LLM, which this head does not hold - build the head with llm_bf16_value_resident=False "
                              "to train")
        dev = self.device
        feat = inputs['mask_features']
        assert feat.shape[0] == 1, 'only support batch size 1 for now.'                     # V4:112
        meta = inputs['img_metas'][0]
        info = meta['masks_info']
        N = len(info)
        names = [object_categories[x['category']] for x in info]                            # V4:116-117
        target = torch.zeros((N, N, self.num_relation_classes))
        for ii, jj, rc in meta['gt_rels'][0]:                                               # V4:122-126
            target[ii, jj, rc] = 1
        binary = (target.sum(2) > 0).float().reshape(-1)
        label_index = torch.nonzero(target, as_tuple=False)
        q = self.cfg.qformer
        # prepare_train (V4:360-406)
        gt_masks = inputs['gt_masks'][0]
        tm = gt_masks.to_tensor(torch.uint8, dev) if hasattr(gt_masks, "to_tensor") else gt_masks.to(dev, torch.uint8)
        sem = inputs['gt_semantic_seg'][0].to(dev).reshape(feat.shape[-2] * 4, feat.shape[-1] * 4).to(torch.int32)
        is_thing = torch.tensor([1 if x['is_thing'] else 0 for x in info], dtype=torch.int32, device=dev)
        cat = torch.tensor([x['category'] for x in info], dtype=torch.int32, device=dev)
        tidx = torch.tensor(np.cumsum([1 if x['is_thing'] else 0 for x in info]) - 1, dtype=torch.int32, device=dev)
        gh, gw = feat.shape[-2] // self.cfg.patch_size, feat.shape[-1] // self.cfg.patch_size
        bits = ops.train_object_bitmasks(tm.contiguous(), sem.contiguous(), is_thing, cat, tidx.clamp(min=0), (gh, gw))
        # sampled pairs (V4:172-186); prompts are padded over ALL pairs (V4:146-150)
        if sampled is None:
            sampled = self.qformer_sampler(target)
        sampled = torch.as_tensor(sampled, dtype=torch.int64)
        uidx, U, tab, tlen = self._prompt_table("q", names)
        rows = [tab[r, :tlen[r]] for r in range(U * U)]
        T = max(len(rows[uidx[i] * U + uidx[j]]) for i in range(N) for j in range(N))
        ids = np.zeros((len(sampled), T), dtype=np.int32)
        msk = np.zeros((len(sampled), T), dtype=np.uint8)
        for r, p in enumerate(sampled.tolist()):
            tok = rows[uidx[p // N] * U + uidx[p % N]]
            ids[r, :len(tok)] = tok
            msk[r, :len(tok)] = 1
        # LLM selection (V4:221-228)
        if selected is None:
            selected = [int(x[0]) * N + int(x[1]) for x in label_index.tolist()]
            selected = random.sample(selected, min(len(selected), self.max_llm_forward_num))
            if len(selected) == 0:
                selected = random.sample(list(range(N * N)), min(N * N, self.max_llm_forward_num))
        selected = [int(x) for x in selected]
        K = len(selected)
        nv = q.num_query
        where = {int(p): r for r, p in enumerate(sampled.tolist())}
        # prompts (left padded, V4:262) and labels ' {name} </s>' per predicate (right padded, V4:267-281)
        tl = target.reshape(-1, self.num_relation_classes).tolist()
        labels = ["".join(" {} </s>".format(self.relation_classes[r]) for r, e in enumerate(tl[si]) if e)
                  for si in selected]
        tok = self.llm_tokenizer
        tok.padding_side = 'left'
        enc_p = tok([self.llm_instruction.format(names[si // N], names[si % N]) for si in selected],
                    return_tensors="pt", padding=True, return_attention_mask=True)
        tok.padding_side = 'right'
        enc_l = tok(labels, return_tensors="pt", padding=True, return_attention_mask=True)
        p_ids, p_m = np.asarray(enc_p["input_ids"]), np.asarray(enc_p["attention_mask"]).astype(bool)
        l_ids, l_m = np.asarray(enc_l["input_ids"]), np.asarray(enc_l["attention_mask"]).astype(bool)
        Tp = p_ids.shape[1]
        seqs, rope, want_rows, want_lab, counts = [], [], [], [], []
        for i in range(K):
            pv, lv = p_ids[i][p_m[i]], l_ids[i][l_m[i]]
            seqs.append(np.concatenate([pv, lv]).astype(np.int32))
            # positions in the reference's padded sequence: a plain HF forward numbers them 0..T-1 over the pads
            ppos = nv + np.nonzero(p_m[i])[0]
            lpos = nv + Tp + np.nonzero(l_m[i])[0]
            rope.append(np.concatenate([np.arange(nv), ppos, lpos]).astype(np.int32))
            for t in range(len(lv) - 1):                        # logits[-Tl:-1] against labels[1:] (V4:337-339)
                want_rows.append((i, nv + len(pv) + t))
                want_lab.append(int(lv[t + 1]))
            counts.append(max(len(lv) - 1, 0))
        Tc = max(len(s_) for s_ in seqs)
        S = nv + Tc
        cids = np.full((K, Tc), -1, dtype=np.int32)
        rpos = np.full((K, S), -1, dtype=np.int32)
        for i in range(K):
            cids[i, :len(seqs[i])] = seqs[i]
            rpos[i, :len(rope[i])] = rope[i]
        return dict(feat=feat, N=N, names=names, binary=binary, bits=bits, sampled=sampled, selected=selected, where=where,
                    mc_label=target.reshape(-1, self.num_relation_classes)[sampled].contiguous(),   # V4:128-129, 198-201
                    ids=torch.from_numpy(ids).to(dev), msk=torch.from_numpy(msk).to(dev), K=K, S=S,
                    cids=torch.from_numpy(cids).to(dev), rpos=torch.from_numpy(rpos).to(dev),
                    seq_len=torch.tensor([nv + len(s_) for s_ in seqs], dtype=torch.int32, device=dev),
                    flat_rows=torch.tensor([i * S + r for i, r in want_rows], dtype=torch.int32, device=dev),
                    want_lab=torch.tensor(want_lab, dtype=torch.int32, device=dev), counts=counts)

    @staticmethod
    def _mean_per_pair(rl, counts):
        per_pair, o = [], 0
        for c in counts:                                         # CrossEntropyLoss(reduction='mean') per pair (V4:339)
            per_pair.append(rl[o:o + c].mean() if c else rl.new_tensor(float("nan")))
            o += c
        return per_pair

    @torch.no_grad()
    def forward_train(self, inputs, sampled=None, selected=None):
        """V4:114-133, 176-196, 218-228, 260-341, 360-406: the two losses of the training branch, computed by the
        inference kernels - `binary_rel_cls_loss` (BCE-with-logits x rel_cls_loss_weight over the sampled pairs) and
        `rel_llm_loss` (teacher-forced next-token cross entropy over the label tokens, mean over the selected pairs).
        Loss VALUES only (validation, checking a checkpoint against the reference; any activation dtype); the losses
        with their gradients come from `forward_train_grad`."""
        dev = self.device
        t = self._train_prepare(inputs, sampled, selected)
        eng = self.rq_engine
        q = self.cfg.qformer
        N, K, S = t["N"], t["K"], t["S"]
        patches = eng.patch_embed(t["feat"].to(torch.float32))
        kv = eng.cross_kv(patches)
        mc = None
        if self.has_multiclass:
            Sn, R = len(t["sampled"]), self.num_relation_classes
            mc = (torch.empty((Sn, R), device=dev, dtype=torch.float32), torch.empty((Sn, R), device=dev, dtype=torch.float32))
        hidden, logit, _ = eng.forward_pairs(kv, t["bits"], N, t["sampled"].to(dev, torch.int32), t["ids"], t["msk"], mc=mc)
        losses = {}
        if self.has_binary:
            losses["binary_rel_cls_loss"] = ops.bce_with_logits(logit, t["binary"][t["sampled"]].to(dev),
                                                                self.rel_cls_loss_weight)   # V4:186-196, 463-482
        if self.has_multiclass:                                   # V4:196-204, 473-477: self-weighted MLCCE rows
            rows = ops.mlcce_rows(mc[0], t["mc_label"].to(dev))
            losses["multiclass_rel_cls_loss"] = torch.mean(rows * (rows / rows.max())) * self.rel_cls_loss_weight
        # pair features of the selected pairs; pairs the sampler skipped stay zero (V4:177, 186)
        nv = q.num_query
        where = t["where"]
        grow = torch.tensor([[where[si] * q.q_rows + 1 + v if si in where else -1 for v in range(nv)]
                             for si in t["selected"]], dtype=torch.int32, device=dev).reshape(-1)
        pf = torch.empty((K * nv, q.hidden), device=dev, dtype=self.act_dtype)
        ops.gather_rows(hidden, grow, pf)
        llm = self.llm_engine
        X = llm.build_inputs(pf, t["cids"], None)
        logits = llm.teacher_forcing_logits(X, t["seq_len"], t["rpos"].reshape(-1), t["flat_rows"])
        rl = ops.cross_entropy_rows(logits.contiguous(), t["want_lab"])
        per_pair = self._mean_per_pair(rl, t["counts"])
        llm_loss = torch.stack(per_pair).mean()                                              # V4:350-351
        self.last = dict(sampled=t["sampled"], selected=t["selected"], bits=t["bits"], bce_logit=logit, llm_logits=logits,
                         llm_row_loss=rl, llm_pair_loss=per_pair, mc_logit=None if mc is None else mc[0])
        return dict(**losses, rel_llm_loss=llm_loss)                                        # V4:345-351

    def forward_train_grad(self, inputs, sampled=None, selected=None, dropout=None):
        """The training branch WITH its gradient graph (V4:327-351, 463-482; tools/train.py:239-246 back-propagates the
        sum of the two losses): the same arithmetic through `openpsg_amd/train_graph.py` - torch.autograd nodes whose
        forward / backward are the fp32 kernels of csrc/psg_train_bwd.hip (its norms, GELU, gate and rotary: the templates
        of csrc/psg_train_rows.h), library GEMMs for the projections.  Gradients
        reach patch_embed, the Q-Former, relation_query / rel_cls_query, binary_rel_cls_pred and language_projection;
        the LLM is frozen (CFG:65) and only passes the gradient through.  fp32 heads - or, with train_precision='bf16', a
        head of any dtype: the same nodes then call the bf16 entry points of csrc/psg_train_bf16.hip (the same templates
        at 16-byte accesses, the attention on the matrix cores) in the bf16 model of DESIGN 13 (bf16 activations
        and products, fp32 residual streams / statistics / losses, fp32 gradients on the fp32 masters).
        dropout: None = `train_dropout` (on by default: the reference trains its Q-Former with HF's default dropouts
        active, V4:78-84); False = off (what the oracle and the goldens are captured with); or a train_graph.Dropout."""
        from . import train_graph as G
        prec = self.train_precision
        if prec is None and self.act_dtype != torch.float32:
            raise PsgHipError("forward_train_grad: the gradient path runs in fp32 (construct the head with dtype='fp32', or "
                              "with train_precision='bf16')")
        dev = self.device
        q = self.cfg.qformer
        with torch.enable_grad():
            P = dict(self.named_parameters())
            if not any(p.requires_grad for p in P.values()):       # (a caller may freeze part of the head; not all of it)
                raise PsgHipError("forward_train_grad: every parameter of the head is frozen (requires_grad False)")
            t = self._train_prepare(inputs, sampled, selected)
            N, K, S = t["N"], t["K"], t["S"]
            feat = t["feat"].to(torch.float32)
            patches = G.PatchEmbedFn.apply(feat, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], self.cfg.patch_size)
            # object masks of the sampled pairs from the packed bits (V4:400-405)
            L = patches.shape[0]
            sh = torch.arange(64, device=dev, dtype=torch.int64)
            om = ((t["bits"][:, :, None] >> sh) & 1).reshape(N, -1)[:, :L].to(torch.uint8)
            sp = t["sampled"].to(dev)
            keep = om[sp // N] | om[sp % N]
            if dropout is None:
                dropout = self.train_dropout
            if dropout is True:
                dropout = G.Dropout(q.hidden_dropout, q.attn_dropout)
            h = G.qformer_pairs(P, self.cfg, patches, t["ids"].to(torch.int64), t["msk"], keep, dropout or None, prec)
            out_s = h[:, :q.q_rows]                                                          # V4:185
            losses, logit, mc_logit = {}, None, None
            if self.has_binary:
                logit = G.linear(out_s[:, 0], P["binary_rel_cls_pred.weight"], P["binary_rel_cls_pred.bias"], prec)
                logit = logit.squeeze(1).float()                                         # the losses take fp32 logits
                losses["binary_rel_cls_loss"] = G.BceFn.apply(logit, t["binary"][t["sampled"]].to(dev),
                                                              self.rel_cls_loss_weight)
            if self.has_multiclass:                                                          # V4:196-204, 473-477
                mc_logit = G.linear(out_s[:, 0], P["multiclass_rel_cls_pred.weight"], P["multiclass_rel_cls_pred.bias"],
                                    prec).float()
                losses["multiclass_rel_cls_loss"] = G.multiclass_loss(mc_logit, t["mc_label"].to(dev),
                                                                      self.rel_cls_loss_weight)
            # pair features of the selected pairs as the reference builds them (V4:177, 186): a zero table of all N*N pairs,
            # `table[sampled] = out`.  The sampler draws WITH replacement (V4:437-461), and index_put's backward hands
            # every duplicate row the gradient of its table entry - so a selected pair that was drawn d times sends the
            # LLM-loss gradient into all d of its rows (the rows hold identical values, whichever lands in the table)
            nv = q.num_query
            table = out_s.new_zeros((N * N, q.q_rows, q.hidden))
            table = table.index_put((sp.to(torch.int64),), out_s)
            pf = table[torch.tensor(t["selected"], dtype=torch.int64, device=dev), 1:]
            vis = G.linear(pf, P["language_projection.weight"], P["language_projection.bias"], prec)         # V4:294
            llm = self.llm_engine if prec is None else self._train_llm()
            cids = t["cids"].to(torch.int64)
            tokv = llm.embed[cids.clamp(min=0)] * (cids >= 0)[..., None].to(vis.dtype)      # frozen embeddings (V4:296)
            X = torch.cat([vis, tokv], dim=1)
            logits = G.llama_teacher_forcing(llm, self.cfg, X, t["seq_len"], t["rpos"], t["flat_rows"].to(torch.int64), prec)
            rl = G.CrossEntropyRowsFn.apply(logits, t["want_lab"])
            per_pair = self._mean_per_pair(rl, t["counts"])
            llm_loss = torch.stack(per_pair).mean()                                          # V4:350-351
        self.last = dict(sampled=t["sampled"], selected=t["selected"], bits=t["bits"],
                         bce_logit=None if logit is None else logit.detach(), llm_logits=logits.detach(),
                         llm_row_loss=rl.detach(), llm_pair_loss=[x.detach() for x in per_pair],
                         mc_logit=None if mc_logit is None else mc_logit.detach())
        return dict(**losses, rel_llm_loss=llm_loss)                                        # V4:345-351

    def train(self, mode: bool = True):
        """The training flag only; `requires_grad` is NOT tied to it (set once at construction: fp32 masters are
        trainable, a caller's freezes stay).  Either transition drops the packed engine copies, which are rebuilt from
        the masters at their next use (the engines also notice in-place updates of the masters by themselves, see
        `_param_version`); the LLM stays frozen (CFG:65)."""
        super().train(mode)
        self._rq_engine = None
        self._proj_stale = True
        if not mode:
            self._train_llm_copy = None                           # the bf16 training copy of the frozen LLM, if one was made
        return self

    def _train_llm(self):
        """The frozen LLM as train_precision='bf16' reads it: the decode engine's own tensors when it holds them in bf16,
        else a bf16 copy made at the first training step and dropped by train(False).  FP8-quantised weights
        (llm_weight_quant='fp8') train on W' = q s rounded to bf16."""
        eng = self.llm_engine
        if eng.dtype == torch.bfloat16:
            return eng
        if self._train_llm_copy is None:
            from types import SimpleNamespace
            b = lambda t: t.to(torch.bfloat16)                   # noqa: E731
            self._train_llm_copy = SimpleNamespace(
                embed=b(eng.embed), lm_head=b(eng.lm_head), final_norm=eng.final_norm, rope=eng.rope,
                layers=[dict(wqkv=b(L["wqkv"]), wo=b(L["wo"]), wgu=b(L["wgu"]), wdown=b(L["wdown"]), ln1=L["ln1"],
                             ln2=L["ln2"]) for L in eng.layers])
        return self._train_llm_copy

    def forward_batch(self, batch):
        """Throughput mode for several images (the reference handles one image per call, V4:112): the
        relation query runs per image, then the selected pairs of ALL images are decoded in one batched
        greedy decode, so the Llama weights stream from HBM once per step for the whole batch instead
        of once per image.  Per-image results are those of forward() up to the rounding of the
        projection GEMMs, which see a different row count (library GEMM above 32 rows).
        (Two BATCHES in flight on two streams were tried and are not offered: above 32 rows the decode projections are
        library GEMMs, and two of those side by side - one in a graph, one eager - hung the GPU at 40 and 80 rows;
        tools/inflight_stress.py batch.)"""
        if self.training:
            raise NotImplementedError("training branch (V4:114-133, 360-406) is out of scope of this build")
        if self.llm_beam_width > 1:
            raise PsgHipError(f"forward_batch decodes one relation per pair; llm_beam_width={self.llm_beam_width} runs through "
                              "forward / submit")
        if self.llm_rel_scores != "constant":
            raise PsgHipError("forward_batch scores LLM triples with the constant 1 only; llm_rel_scores='likelihood' runs "
                              "through forward / submit")
        st, gslot = torch.cuda.current_stream(self.device), 0
        items, results, tokens, mcs = [], [None] * len(batch), None, {}
        with torch.cuda.stream(st):
            for i, inputs in enumerate(batch):
                feat, meta, info, obj_ids, names = self._unpack(inputs)
                if not obj_ids:
                    results[i] = dict(rel_pred=[], rel_score=[])
                    continue
                rq = self.run_relation_query(feat, meta, obj_ids, names, info["pan_results"])
                if self.has_multiclass:
                    mcs[i] = (rq["mc_topk"], len(obj_ids))
                if not self.has_binary:
                    continue
                X, plen = self.llm_inputs(rq, names)
                items.append((i, len(obj_ids), rq["selected"], X, plen))
            if items:
                maxlen = max(it[3].shape[1] for it in items)
                Xs = []
                for _, _, _, X, _ in items:                              # rows past a pair's length are never read
                    if X.shape[1] < maxlen:
                        X = torch.cat([X, X.new_zeros((X.shape[0], maxlen - X.shape[1], X.shape[2]))], dim=1)
                    Xs.append(X)
                Xall, pall = torch.cat(Xs), torch.cat([it[4] for it in items])
                if Xall.shape[0] % 4:                                    # data-dependent pair counts: keep the decode
                    extra = 4 - Xall.shape[0] % 4                        # graphs few (copies of the last pair, cut below)
                    Xall = torch.cat([Xall, Xall[-1:].expand(extra, -1, -1)])
                    pall = torch.cat([pall, pall[-1:].expand(extra)])
                tokens = self.llm_engine.generate(Xall, pall, suppress_eos=self.suppress_eos, slot=gslot,
                                                  constraint=self._constraint())
        return _PendingBatch(self, st, items, results, tokens, mcs).result()

    def image_constants(self, feat, meta, obj_ids, pan):
        """What the rank that holds an image's segmenter outputs hands to the other ranks: the patch
        embedding [L, C] fp32 (V4:410; 256 KB instead of the 67 MB feature map) and the object bitmasks
        [N, ceil(L/64)] (V4:416-429).  With the object ids - from which every rank derives the names and looks the
        prompt ids up in its own per-class-pair tables (V4:146-152) - that is all `run_relation_query` needs."""
        eng = self.rq_engine
        patches = eng.patch_embed(feat.to(torch.float32))
        ids_dev = torch.tensor(obj_ids, dtype=torch.int32, device=self.device)
        pan_dev = pan.to(device=self.device, dtype=torch.int32).contiguous()
        return patches, eng.object_bitmasks(pan_dev, meta, ids_dev, feat.shape[-2:])

    def _prepare_image(self, feat, meta, obj_ids, names, pan, patches=None, bits=None):
        """A4 + A5 for one image: shared cross-attention K/V, object bitmasks, prompt-id table (cached per names).
        bits given (another rank computed them, `image_constants`): `feat`, `meta` and `pan` are not touched."""
        eng = self.rq_engine
        dev = self.device
        N = len(obj_ids)
        if patches is None:
            patches = eng.patch_embed(feat.to(torch.float32))
        kv = eng.cross_kv(patches)
        if bits is None:
            # pinned staging + non_blocking: a pageable host-to-device copy waits for the stream to drain (a host wait in
            # the middle of `submit`)
            ids_dev = torch.tensor(obj_ids, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            pan_dev = pan.to(device=dev, dtype=torch.int32).contiguous()
            bits = eng.object_bitmasks(pan_dev, meta, ids_dev, feat.shape[-2:])
        # BERT prompts: [U*U, T] table gathered per pair on the device (cached per set of names)
        ck = ("q", tuple(names))
        if ck not in self._table_cache:
            uidx, U, tab, tlen = self._prompt_table("q", names)                             # every class pair occurs: i, j
            T = int(tlen.max())                                                             # range over all objects
            msk = (np.arange(T)[None, :] < tlen[:, None])                                   # padding=True
            tbl = np.where(msk, tab[:, :T], 0).astype(np.int32)
            msk = msk.astype(np.uint8)
            if len(self._table_cache) > 64:
                self._table_cache.clear()
            self._table_cache[ck] = (np.asarray(uidx, dtype=np.int64), U, torch.from_numpy(tbl).to(dev),
                                     torch.from_numpy(msk).to(dev), torch.tensor(uidx, dtype=torch.int64, device=dev))
        return patches, kv, bits, ck

    def _chunk_prompts(self, ck, N, c0, c1):
        """(pair ids int32 [c1-c0], BERT ids [c1-c0, T], mask) of the pairs c0..c1-1; depends on the names only."""
        gk = (ck, N, c0, c1)
        ent = self._gather_cache.get(gk)
        if ent is None:
            uidx, U, tbl_d, msk_d, u_d = self._table_cache[ck]
            pidx = torch.arange(c0, c1, device=self.device, dtype=torch.int64)
            trow = u_d[pidx // N] * U + u_d[pidx % N]
            if len(self._gather_cache) > 64:
                self._gather_cache.clear()
            # the distinct prompts among these pairs and every pair's row in that table (the engine runs the
            # prompt-only part of the Q-Former once per distinct prompt): a few host array operations, no device
            # round trip
            ph = np.arange(c0, c1, dtype=np.int64)
            uniq_h, inv_h = np.unique(uidx[ph // N] * U + uidx[ph % N], return_inverse=True)
            uniq = torch.from_numpy(uniq_h).to(self.device)
            # (ids, mask) of the distinct prompts, every pair's row in that table, and - names-only index arithmetic the
            # engine would otherwise redo on the device for every image - the 33 query rows of each pair's prompt block
            nq = self.cfg.qformer.q_rows
            rows33 = (inv_h.astype(np.int64)[:, None] * nq + np.arange(nq)[None, :]).reshape(-1).astype(np.int32)
            prompts = (tbl_d[uniq].contiguous(), msk_d[uniq].contiguous(),
                       torch.from_numpy(inv_h.astype(np.int32)).to(self.device), torch.from_numpy(rows33).to(self.device))
            ent = self._gather_cache[gk] = (pidx.to(torch.int32), tbl_d[trow].contiguous(), msk_d[trow].contiguous(),
                                            prompts)
        return ent

    def run_relation_query(self, feat, meta, obj_ids, names, pan, pair_range=None, patches=None, bits=None):
        """A4-A8 on the GPU.  pair_range=(p0,p1) restricts the Q-Former to a shard of the pairs;
        `patches` [L,C] fp32 skips the patch embedding (pair sharding: another rank computed it); with `bits` as well
        (`image_constants` of that rank) feat / meta / pan may be None: this rank never sees the image."""
        eng = self.rq_engine
        dev = self.device
        N = len(obj_ids)
        B = N * N
        patches, kv, bits, ck = self._prepare_image(feat, meta, obj_ids, names, pan, patches, bits)
        uidx = self._table_cache[ck][0].tolist()
        p0, p1 = (0, B) if pair_range is None else pair_range
        q = self.cfg.qformer
        single = 0 < p1 - p0 <= self.pair_chunk                  # one chunk: take the engine's outputs as they are
        mc = None
        if self.has_multiclass:
            if pair_range is not None:
                raise PsgHipError("the multiclass head runs over all pairs of an image (no pair_range)")
            # every chunk writes its rows of ONE [N^2, R] buffer (probabilities of the diagonal pairs already 0)
            R = self.num_relation_classes
            mc = (torch.empty((B, R), device=dev, dtype=torch.float32), torch.empty((B, R), device=dev, dtype=torch.float32))
        mcs = lambda c0, c1: None if mc is None else (mc[0][c0:c1], mc[1][c0:c1])  # noqa: E731
        if self.cls_first and p1 > p0:
            # selection phase first (per chunk of pairs), the selected pairs' rows 1..32 on demand
            pending, lgs, prs = [], [], []
            for c0 in range(p0, p1, self.pair_chunk):
                c1 = min(p1, c0 + self.pair_chunk)
                ent = self._chunk_prompts(ck, N, c0, c1)
                state, lg, pr = eng.forward_pairs_cls(kv, bits, N, ent[0], ent[1], ent[2], prompts=ent[3], mc=mcs(c0, c1))
                pending.append((c0, c1, state, 0))
                lgs.append(lg)
                prs.append(pr)
            if self.has_binary:
                logit, prob = (lgs[0], prs[0]) if len(lgs) == 1 else (torch.cat(lgs), torch.cat(prs))
            else:
                logit = prob = None
            out = _LazyRQ(patches=patches, bits=bits, exist_logit=logit, exist_prob=prob, num_objects=N,
                          pair_range=(p0, p1), uidx=uidx, pending=pending)
            out.engine = eng
            if pair_range is None:
                out["selected"] = self.select_pairs(prob, N) if self.has_binary else None
            self._multiclass_topk(out, mc)
            return out
        if not single:
            np_ = max(0, p1 - p0)                                 # an empty shard (more ranks than pairs) is legal
            hidden = torch.empty((np_ * q.q_rows, q.hidden), device=dev, dtype=self.act_dtype)
            logit = torch.empty(np_, device=dev, dtype=torch.float32) if self.has_binary else None
            prob = torch.empty(np_, device=dev, dtype=torch.float32) if self.has_binary else None
        for c0 in range(p0, p1, self.pair_chunk):
            c1 = min(p1, c0 + self.pair_chunk)
            ent = self._chunk_prompts(ck, N, c0, c1)
            if single:
                hidden, logit, prob = eng.forward_pairs(kv, bits, N, ent[0], ent[1], ent[2], mc=mcs(c0, c1))
            else:                                                 # the last layer writes straight into its slice
                _, lg, pr = eng.forward_pairs(kv, bits, N, ent[0], ent[1], ent[2],
                                              hidden_out=hidden[(c0 - p0) * q.q_rows:(c1 - p0) * q.q_rows],
                                              mc=mcs(c0, c1))
                if self.has_binary:
                    logit[c0 - p0:c1 - p0] = lg
                    prob[c0 - p0:c1 - p0] = pr
        out = dict(patches=patches, bits=bits, hidden=hidden, exist_logit=logit, exist_prob=prob,
                   num_objects=N, pair_range=(p0, p1), uidx=uidx)
        if pair_range is None:
            out["selected"] = self.select_pairs(prob, N) if self.has_binary else None
        self._multiclass_topk(out, mc)
        return out

    def _multiclass_topk(self, out, mc):
        """V4:238-257 with the SURVEY 0.3 corrections, on the device: the k = min(num_multiclass_triples, N^2 R) best
        flat indices f = p R + r of the [N^2, R] probabilities (diagonal already 0; psg_topk's order) as ONE int32 [2, k]
        tensor - row 0 the indices, row 1 the fp32 scores' bits - so that the host fetches both with a single copy."""
        if mc is None:
            return
        n = mc[1].numel()
        k = min(self.num_multiclass_triples, n)
        res = torch.empty((2, k), device=mc[1].device, dtype=torch.int32)
        ws = torch.empty(ops.topk_large_workspace_bytes(mc[1].device, n, k), device=mc[1].device, dtype=torch.uint8)
        ops.topk_large(mc[1].view(-1), k, ws, idx=res[0], val=res[1].view(torch.float32))
        out.update(mc_logit=mc[0], mc_prob=mc[1], mc_topk=res)

    def parse_multiclass(self, mc_host, object_num):
        """Host side of `_multiclass_topk`: the kept flat indices f -> triples [p // N, p % N, r] (p = f // R, r = f % R)
        with their scores as Python floats.  The indices are distinct, so are the triples (V4:255-257 keeps the first
        occurrence of a triple)."""
        if mc_host is None:
            return [], []
        R = self.num_relation_classes
        idx, val = mc_host[0], mc_host[1].view(np.float32)
        rel_pred, rel_score = [], []
        for f, v in zip(idx.tolist(), val.tolist()):
            if f < 0:
                break
            p = f // R
            rel_pred.append([p // object_num, p % object_num, f % R])
            rel_score.append(float(v))
        return rel_pred, rel_score

    def run_relation_query_shards(self, items, pair_range, patches_list):
        """Pair sharding over R images: a shard of EVERY image in one Q-Former pass - the dense projections
        see all the images' shard pairs at once (as many rows as one whole image), only the cross-attention runs per
        image (its K/V and object masks are per image).  items[m] = (feat, meta, obj_ids, names, pan); pair_range:
        one (p0, p1) for all images or a list with image m's own range (images with different object counts).
        Returns [(hidden_m or pending handle, exist_prob_m [p1_m - p0_m])]."""
        eng = self.rq_engine
        ranges = [tuple(pair_range)] * len(items) if isinstance(pair_range, tuple) else [tuple(rg) for rg in pair_range]
        Ps = [max(0, p1 - p0) for p0, p1 in ranges]
        if min(Ps) <= 0 or sum(Ps) > self.pair_chunk or len(items) < 4:   # measured: 8 images 7.0 -> 6.4 ms, 2 images no gain
            outs = []
            for (feat, meta, obj_ids, names, pan), patches, rg in zip(items, patches_list, ranges):
                if len(obj_ids) == 0:
                    outs.append((torch.zeros((0, self.cfg.qformer.hidden), device=self.device, dtype=self.act_dtype),
                                 torch.zeros(0, device=self.device)))
                    continue
                rq = self.run_relation_query(feat, meta, obj_ids, names, pan, pair_range=rg, patches=patches)
                outs.append((rq if "pending" in rq else rq["hidden"], rq["exist_prob"]))
            return outs
        segs, pidx, ids, msk, off = [], [], [], [], 0
        for m, ((feat, meta, obj_ids, names, pan), patches) in enumerate(zip(items, patches_list)):
            _, kv, bits, ck = self._prepare_image(feat, meta, obj_ids, names, pan, patches)
            ent = self._chunk_prompts(ck, len(obj_ids), ranges[m][0], ranges[m][1])
            segs.append((off, Ps[m], kv, bits, len(obj_ids)))
            off += Ps[m]
            pidx.append(ent[0])
            ids.append(ent[1])
            msk.append(ent[2])
        T = max(t.shape[1] for t in ids)                          # prompts of different images pad to the longest
        pad = lambda t: t if t.shape[1] == T else torch.cat([t, t.new_zeros((t.shape[0], T - t.shape[1]))], dim=1)  # noqa: E731
        if self.cls_first:
            state, logit, prob = eng.forward_pairs_cls(None, None, None, torch.cat(pidx), torch.cat([pad(t) for t in ids]),
                                                       torch.cat([pad(t) for t in msk]), segments=segs)
            outs = []
            for m, (ps, pc, kv_m, bits_m, n_m) in enumerate(segs):
                st_m = dict(state, kv=kv_m, bits=bits_m, num_objects=n_m, segments=None)   # image m's view of the pass
                rq = _LazyRQ(exist_logit=logit[ps:ps + pc], exist_prob=prob[ps:ps + pc], num_objects=n_m,
                             pair_range=ranges[m], pending=[(ranges[m][0], ranges[m][1], st_m, ps)])
                rq.engine = eng
                outs.append((rq, rq["exist_prob"]))
            return outs
        hidden, _, prob = eng.forward_pairs(None, None, None, torch.cat(pidx), torch.cat([pad(t) for t in ids]),
                                            torch.cat([pad(t) for t in msk]), segments=segs)
        q_rows = self.cfg.qformer.q_rows
        return [(hidden[ps * q_rows:(ps + pc) * q_rows], prob[ps:ps + pc]) for ps, pc, _, _, _ in segs]

    def select_pairs(self, prob, N):
        """A8.  'topk': first num_selected of the full descending order (V4:235-237).  'threshold'
        (V4:230-234, commented out in the reference): every pair with p > pair_selector_threshold,
        topped up to at least max_llm_forward_num by score, capped at max_selected; the count is
        data dependent, so this costs one scalar device->host read."""
        eng = self.rq_engine
        B = N * N
        if self.exclude_diagonal:
            prob = prob.clone()
            prob[torch.arange(N, device=prob.device) * (N + 1)] = -1.0
        if self.pair_selector == "topk":
            return eng.select(prob, min(self.cfg.num_selected, B))
        cap = min(self.max_selected, B)
        order = eng.select(prob, cap)
        n_hit = int((prob > self.pair_selector_threshold).sum().item())
        k = max(1, min(cap, max(n_hit, min(self.max_llm_forward_num, B))))
        return order[:k].contiguous()

    def selected_pair_features(self, rq, selected=None, zero_foreign=False):
        """pair_feature = hidden[:, 1:] (V4:215) of the selected pairs, [K*32, 768].  zero_foreign: pairs outside the
        rq's pair range (another rank's shard; negative ids) give zero rows instead of being an error."""
        sel = rq["selected"] if selected is None else selected
        q = self.cfg.qformer
        K, nv = sel.numel(), q.num_query
        if "pending" in rq and "hidden" not in rq:
            # selection phase done (forward_pairs_cls): last layer in full for the K chosen pairs only.  Several
            # chunks: every chunk computes all K slots (foreign pairs as its first pair) and keeps its own - no host sync
            pf = torch.zeros((K, nv, q.hidden), device=self.device, dtype=self.act_dtype) if zero_foreign else None
            for c0, c1, st, off in rq["pending"]:
                if st.get("segments") is None:
                    # one kernel gathers the selected pairs' rows, masks and pair ids (foreign slots: the chunk's own
                    # first pair, flagged) - no selection-dependent index arithmetic on the device
                    hk, mine_u8 = self.rq_engine.pair_hidden_sel(st, sel, c0, c1 - c0, off)
                    pc = hk.view(K, q.q_rows, q.hidden)[:, 1:]
                    if pf is None and len(rq["pending"]) == 1:
                        pf = pc                                            # single chunk, every pair its own
                    else:
                        pf = pc if pf is None else torch.where(mine_u8.bool()[:, None, None], pc, pf)
                    continue
                local = sel.to(torch.int64) - c0
                mine = (local >= 0) & (local < c1 - c0)
                # foreign slots are computed as this chunk's FIRST pair (a valid pair of the same image: in a pass over
                # several images position 0 belongs to another image, whose pair ids can exceed this image's N^2)
                pos = torch.where(mine, local + off, torch.full_like(local, off)).to(torch.int32)
                hk = self.rq_engine.pair_hidden(st, pos)
                pc = hk.view(K, q.q_rows, q.hidden)[:, 1:]
                pf = pc if pf is None else torch.where(mine[:, None, None], pc, pf)
            return pf.reshape(K * nv, q.hidden)
        p0, p1 = rq.get("pair_range", (0, rq["num_objects"] ** 2))   # `hidden` holds the pairs [p0, p1)
        local = sel.to(torch.int64) - p0
        rows = local[:, None] * q.q_rows + 1 + torch.arange(nv, device=self.device)[None, :]
        if zero_foreign:                                              # psg_gather_rows writes zeros for index < 0
            rows = torch.where(((local >= 0) & (local < p1 - p0))[:, None], rows, torch.full_like(rows, -1))
        pf = torch.empty((K * nv, q.hidden), device=self.device, dtype=self.act_dtype)
        ops.gather_rows(rq["hidden"], rows.reshape(-1).to(torch.int32), pf)
        return pf

    def selected_pair_features_multi(self, rqs, selected):
        """`selected_pair_features(..., zero_foreign=True)` for several images whose shards went through ONE
        selection-phase pass (`run_relation_query_shards`): one last-layer pass over all images' slots instead of
        one per image.  rqs[m] / selected[m]: image m's handle and its K selected pair ids.  Returns a list of
        [K*32, 768] tensors; falls back to per-image calls when the handles do not share a pass."""
        q = self.cfg.qformer
        nv = q.num_query
        ok = all("pending" in r and "hidden" not in r and len(r["pending"]) == 1 for r in rqs)
        if ok:
            base = rqs[0]["pending"][0][2].get("X")                 # one shared multi-image pass (never prompt-deduplicated)
            ok = base is not None and all(r["pending"][0][2].get("X") is base for r in rqs)
        if not ok or len(rqs) == 1:
            return [self.selected_pair_features(r, s, zero_foreign=True) for r, s in zip(rqs, selected)]
        pos, mine_all, segs, k0 = [], [], [], 0
        for r, sel in zip(rqs, selected):
            c0, c1, st, off = r["pending"][0]
            local = sel.to(torch.int64) - c0
            mine = (local >= 0) & (local < c1 - c0)
            pos.append(torch.where(mine, local + off, torch.full_like(local, off)))   # foreign: the image's own first pair
            mine_all.append(mine)
            segs.append((k0, sel.numel(), st["kv"], st["bits"], st["num_objects"]))
            k0 += sel.numel()
        st0 = rqs[0]["pending"][0][2]
        hk = self.rq_engine.pair_hidden(st0, torch.cat(pos).to(torch.int32), segments=segs)
        pf = hk.view(k0, q.q_rows, q.hidden)[:, 1:]
        pf = torch.where(torch.cat(mine_all)[:, None, None], pf, torch.zeros_like(pf))
        outs, k0 = [], 0
        for sel in selected:
            outs.append(pf[k0:k0 + sel.numel()].reshape(sel.numel() * nv, q.hidden))
            k0 += sel.numel()
        return outs

    def llm_inputs(self, rq, names, selected=None, pair_features=None):
        """V4:240-301: LLM input embeddings X [K, 32+Tp, D] and prompt lengths [K] of the selected pairs.
        `pair_features` [K*32, 768] replaces the gather from rq["hidden"] (pair sharding: the features
        arrive by reduce-scatter)."""
        dev = self.device
        N = rq["num_objects"]
        sel = rq["selected"] if selected is None else selected
        K = sel.numel()
        q = self.cfg.qformer
        nv = q.num_query
        pf = self.selected_pair_features(rq, sel) if pair_features is None else pair_features
        # Llama prompts, compacted (left padding of V4:262 removed; see llm.py); cached per set of names
        ck = ("l", tuple(names))
        if ck not in self._table_cache:
            uidx, U, tab, lens = self._prompt_table("l", names)
            Tp = int(lens.max())
            # the longest prompt changes from image to image (its class names); the prompt grid is rounded up so
            # that the decode graphs, keyed by input shape, are reused (rows past a pair's length carry pos = -1
            # and are skipped by every kernel)
            if self.prompt_bucket > 1:
                Tp = -(-Tp // self.prompt_bucket) * self.prompt_bucket
            tbl = np.full((U * U, Tp), -1, dtype=np.int32)                                 # valid ids first, -1 after
            w = min(Tp, tab.shape[1])
            tbl[:, :w] = tab[:, :w]
            lens = lens.astype(np.int32)
            if len(self._table_cache) > 64:
                self._table_cache.clear()
            self._table_cache[ck] = (uidx, U, torch.from_numpy(tbl).to(dev), torch.from_numpy(lens).to(dev),
                                     torch.tensor(uidx, dtype=torch.int64, device=dev))
        uidx, U, tbl_d, lens_d, u_d = self._table_cache[ck]
        s64 = sel.to(torch.int64)
        trow = u_d[s64 // N] * U + u_d[s64 % N]
        pids, plen = tbl_d[trow].contiguous(), lens_d[trow].contiguous()
        return self.llm_engine.build_inputs(pf, pids, plen), plen

    def decode_selected(self, rq, names, selected=None, pair_features=None, to_host=True, slot=0, gate=None, defer=False):
        """A9: batched greedy decode of the selected pairs.
        defer (`submit`): nothing waits for the GPU here; with natural EOS the chunks behind the first are replayed by
        `out["_finish"]()` (called by the pending result), which also fills `tokens` / `first_logits`."""
        sel = rq["selected"] if selected is None else selected
        K = sel.numel()
        sel_in = sel
        if self.pair_selector == "threshold" and K % 4 and (
                self.llm_beam_width == 1 or (K + 4 - K % 4) * self.llm_beam_width <= 160):      # (a beam stays within 160 rows)
            # the pair count is data dependent here: round it up to a multiple of 4 with copies of the last pair
            # (decode is weight-streaming-bound, extra rows are almost free) so that the engine keeps a few
            # decode graphs instead of one per count
            sel_in = torch.cat([sel, sel[-1:].expand(4 - K % 4)]).contiguous()
            if pair_features is not None:
                nv = self.cfg.qformer.num_query
                pair_features = torch.cat([pair_features, pair_features[-nv:].repeat(4 - K % 4, 1)]).contiguous()
        X, plen = self.llm_inputs(rq, names, sel_in, pair_features)
        eng = self.llm_engine
        # deferring leaves later chunks un-enqueued when the next image's front half starts: only when the decode steps
        # hold own kernels alone (library GEMMs of two streams side by side were seen to hang, `submit`)
        defer = bool(defer) and eng.use_skinny and sel_in.numel() <= 32 and not eng.decode_uses_library(sel_in.numel())
        con = self._constraint()
        scored = self.llm_rel_scores == "likelihood"
        if self.llm_beam_width > 1:                             # the beam's classes and scores are the whole result
            res = eng.generate(X, plen, slot=slot, constraint=con, beam=self.llm_beam_width)
            out = dict(llm_inputs=X[:K], prompt_len=plen[:K], tokens=None,
                       beam_class=res[0][:K], beam_logp=res[1][:K])   # padding copies of the threshold selector are cut here
            if to_host:
                out["beam_class_host"], out["beam_logp_host"] = out["beam_class"].cpu().numpy(), out["beam_logp"].cpu().numpy()
                out["selected_host"] = sel.cpu().numpy()
            return out
        # a constrained decode scores the triple it emits itself: the trie pass (and its cache slots) is needed only for
        # the ranked triples behind it
        trie = self.relation_trie() if scored and (con is None or self.num_llm_ranked_triples > 0) else None
        res = eng.generate(X, plen, suppress_eos=self.suppress_eos, return_first_logits=True, slot=slot, gate=gate,
                           defer=defer, trie=trie, constraint=con, path_logp=scored and con is not None)
        out = dict(llm_inputs=X[:K], prompt_len=plen[:K])

        def finish():
            r = res() if defer else res
            out["tokens"], out["first_logits"] = r[0][:K], r[1][:K]
            if trie is not None:                                # padding copies of the threshold selector are cut here
                out["rel_logscores"] = r[2][:K]
            if scored and con is not None:
                out["path_logp"] = r[-1][:K]
        if defer:
            out["_finish"] = finish
            return out
        finish()
        if to_host:
            out["tokens_host"], out["selected_host"] = out["tokens"].cpu().numpy(), sel.cpu().numpy()
            if trie is not None:
                out["logscores_host"] = out["rel_logscores"].cpu().numpy()
            if out.get("path_logp") is not None:
                out["path_logp_host"] = out["path_logp"].cpu().numpy()
        return out

    def _constraint(self):
        """The trie the decode is constrained to (llm_decode='constrained'), or None."""
        return self.relation_trie() if self.llm_decode == "constrained" else None

    def _parse_out(self, out, N):
        """rel_pred / rel_score of the LLM stage from a decode's host copies."""
        if out.get("beam_class_host") is not None:
            return self.parse_beam(out["beam_class_host"], out["beam_logp_host"], out["selected_host"], N)
        if out.get("path_logp_host") is not None:
            return self.parse_path_scored(out["tokens_host"], out["selected_host"], N, out["path_logp_host"],
                                          out.get("logscores_host"))
        if self.llm_rel_scores == "likelihood":
            return self.parse_scored(out["tokens_host"], out["selected_host"], N, out["logscores_host"])
        return self.parse(out["tokens_host"], out["selected_host"], N)

    def parse(self, tokens_host, selected_host, object_num):
        """A10 (V4:313-326): decode -> text between '<s>' and '</s>' -> names split on two spaces.

        `generate(inputs_embeds=...)` returns only the NEW tokens on current transformers, while the
        reference's `split('<s>')[1]` needs a '<s>' in the decoded text.  Training never teaches the
        model to emit one (the label's BOS is an INPUT: the loss pairs logits[-Tl:-1] with
        labels[1:], V4:327-341), so the sequence the reference parses is the generation behind an
        implicit BOS - which is what the transformers releases that seed `sequences` with a BOS
        token hand to `batch_decode`.  Default `implicit_bos=True`: a text without '<s>' is parsed
        as if it followed one.  `implicit_bos=False` keeps the literal V4:315 behaviour
        (IndexError unless on_parse_error='skip')."""
        rel_pred, rel_score = [], []
        for _, t in self._parse_pairs(tokens_host, selected_host, object_num):
            rel_pred.append(t)
            rel_score.append(1)
        return rel_pred, rel_score

    def _relation_names(self, seq):
        """Class indices (into relation_categories) that V4:313-321 reads from one generated id sequence, in text order;
        None when the text is skipped (no '<s>', implicit_bos=False, on_parse_error='skip')."""
        text = self.llm_tokenizer.batch_decode([seq])[0]
        parts = text.split('<s>')
        if len(parts) > 1:
            body = parts[1]
        elif self.implicit_bos:
            body = parts[0]
        elif self.on_parse_error == "raise":
            raise IndexError("no '<s>' in the generated text (V4:315-316); construct the head with "
                             "implicit_bos=True or on_parse_error='skip'")
        else:
            return None
        pred = body.split('</s>')[0].strip()
        return [relation_categories.index(name) for name in pred.split('  ') if name in relation_categories]

    def _parse_pairs(self, tokens_host, selected_host, object_num):
        """[(selection rank k, [sub, obj, rel])] of V4:313-326, new triples only, in parse order."""
        out, seen = [], []
        for k, si in enumerate(selected_host.tolist()):
            seq = [int(t) for t in tokens_host[k] if t >= 0]
            rels = self._relation_names(seq)
            for r in rels or ():
                t = [si // object_num, si % object_num, r]
                if t not in seen:
                    seen.append(t)
                    out.append((k, t))
        return out

    def parse_scored(self, tokens_host, selected_host, object_num, log_scores):
        """`parse` with llm_rel_scores='likelihood': the generated triples scored s(p, r) = exp(log_scores[k, r]), then
        the num_llm_ranked_triples best remaining (pair, class) triples (rel_scores.assemble)."""
        return assemble(self._parse_pairs(tokens_host, selected_host, object_num), log_scores, selected_host, object_num,
                        self.num_llm_ranked_triples)

    def parse_path_scored(self, tokens_host, selected_host, object_num, path_logp, log_scores=None):
        """`parse` of a constrained decode with llm_rel_scores='likelihood': pair k's triple scored exp(path_logp[k]), the
        probability the decode steps themselves gave its candidate (s(p, r) of DESIGN 11 without the trie pass).
        log_scores [K, R] (the trie pass, num_llm_ranked_triples > 0): the ranked triples follow as in `parse_scored`."""
        pairs = self._parse_pairs(tokens_host, selected_host, object_num)
        own = [float(np.exp(np.float64(path_logp[k]))) for k, _ in pairs]
        if log_scores is None:
            return [list(t) for _, t in pairs], own
        rel_pred, rel_score = assemble(pairs, log_scores, selected_host, object_num, self.num_llm_ranked_triples)
        return rel_pred, own + rel_score[len(own):]

    def parse_beam(self, beam_class, beam_logp, selected_host, object_num):
        """rel_pred / rel_score of a beam decode (llm_beam_width > 1).  beam_class int [K, B] (-1 padded) /
        beam_logp [K, B]: each pair's hypotheses, best first.  First each pair's best hypothesis in selection order - the K
        triples llm_decode='constrained' returns -, then the remaining hypotheses of all pairs by descending score, ties to
        the lower selection rank, then the lower class.  rel_score = exp(logp)."""
        cls, lp = np.asarray(beam_class), np.asarray(beam_logp, dtype=np.float64)
        first, rest = [], []
        for k, si in enumerate(np.asarray(selected_host).tolist()):
            for b in range(cls.shape[1]):
                r = int(cls[k, b])
                if r >= 0:
                    (first if b == 0 else rest).append((k, r, float(lp[k, b]), [si // object_num, si % object_num, r]))
        rest.sort(key=lambda e: (-e[2], e[0], e[1]))
        order = first + rest
        return [e[3] for e in order], [float(np.exp(e[2])) for e in order]

    def relation_trie(self):
        """The token trie of the relation classes' candidate sequences under the current LLM tokenizer (rel_scores.py),
        built and checked at construction and again whenever `llm_tokenizer` is replaced."""
        if self._rel_trie is None or self._rel_trie_tok is not self.llm_tokenizer:
            tok = self.llm_tokenizer

            def parse_classes(ids):
                saved = self.on_parse_error
                try:
                    self.on_parse_error = "skip"
                    return set(self._relation_names(list(ids)) or ())
                finally:
                    self.on_parse_error = saved
            self._rel_trie = build_relation_trie(tok, list(relation_categories), self.cfg.llm.eos, self.cfg.llm.vocab,
                                                 parse_classes)
            self._rel_trie_tok = tok
            if self.llm_decode == "constrained" and self.cfg.max_new_tokens < self._rel_trie.max_depth + 1:
                need, self._rel_trie = self._rel_trie.max_depth + 1, None
                raise PsgHipError(f"llm_decode='constrained': max_new_tokens={self.cfg.max_new_tokens} is below the relation "
                                  f"trie's depth + 1 = {need}: the longest class name could not finish")
        return self._rel_trie
