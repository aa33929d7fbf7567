"""Shared by tests/test_gpu_llm_option_matrix.py and tests/test_llm_option_matrix_cpu.py: the weight variants of the LLM
option matrix, the model W' each of them IS, the relation trie of the 56 PSG classes, and the CPU oracle's own LLM inputs.
Nothing here needs a GPU."""
import numpy as np
import torch

from tests import helpers as H

FORMATS = ("fp8", "mxfp4", "int4g")
G1, G8, G6 = "G1_c1_512_n10", "G8_gqa_512_n10", "G6_llm_7b_width_n6"
# every (case, fmt, lm_head) the matrix decodes on: G1 and G8, unquantised and the three formats with and without the lm_head
VARIANTS = [(case, fmt, lm_head) for case in (G1, G8)
            for fmt, lm_head in [(None, False)] + [(f, h) for f in FORMATS for h in (False, True)]]


def load(case):
    if case.startswith(("G8", "G9")):
        from tests.test_gpu_gqa_head import load_gqa_case
        return load_gqa_case(case)
    return H.load_case(case)


def formats(eng):
    """The format (None, 'fp8', 'mxfp4', 'int4') of every matrix record of the engine: the decoder layers', then the lm_head's."""
    return [rec.fmt for rec in eng.matrices()]


def streams(eng):
    """... and the kind of the stream each has in a decode step of <= 32 rows (None: it runs on W')."""
    return [rec.stream[0] if rec.stream is not None else None for rec in eng.matrices()]


def dequantised(w, n_layers, fmt, lm_head=False):
    """The model a head with llm_weight_quant=fmt computes: W' in fp32 for every quantised matrix (fmt None: w itself)."""
    if fmt is None:
        return w
    from tests.test_gpu_llm_int4 import _dequantised as int4g
    from tests.test_gpu_llm_w4 import _dequantised as mxfp4
    from tests.test_gpu_llm_w8 import _dequantised as fp8
    return dict(fp8=fp8, mxfp4=mxfp4, int4g=int4g)[fmt](w, n_layers, lm_head)


def relation_trie(cfg):
    """The trie `head.relation_trie()` builds for the word tokenizer (equal `key`)."""
    from openpsg_amd.categories import relation_categories
    from openpsg_amd.rel_scores import RelationTrie, candidate_ids
    from openpsg_amd.tokenizers import WordTokenizer
    tok = WordTokenizer("llama")
    return RelationTrie(list(relation_categories), [candidate_ids(tok, n, cfg.llm.eos) for n in relation_categories],
                        cfg.llm.eos)


def oracle_llm_inputs(g, cfg, w, scene):
    """The CPU oracle's own LLM inputs of the golden selection, as tests/test_gpu_llm_w8.py builds them
    (O.relation_query -> O.llm_inputs), compacted to what `_oracle_walk` reads: X [K, S, D] with each pair's valid rows
    first, seq_len [K].  No quantised matrix is read: the inputs are those of every weight variant of the case."""
    from oracle import psg_oracle as O
    sel = g["selected"].tolist()
    qids, qmask = H.qformer_prompts(scene)
    pids, pmask = H.llm_prompts(scene, sel)
    with torch.no_grad():
        orq = O.relation_query(w, cfg, scene["mask_features"], scene["img_meta"], [int(i) for i in scene["object_id_list"]],
                               scene["pan_results"], qids, qmask)
        rows = []
        for i, si in enumerate(sel):
            x, mask = O.llm_inputs(w, orq["pair_feature"][si], pids[i], pmask[i])
            rows.append(x[mask.bool()].float())
    seq_len = np.array([r.shape[0] for r in rows])
    X = torch.zeros((len(rows), int(seq_len.max()), rows[0].shape[1]))
    for k, r in enumerate(rows):
        X[k, :r.shape[0]] = r
    return X, seq_len
