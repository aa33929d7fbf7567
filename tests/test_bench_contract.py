"""bench.py's hand-off of figures that are READ from committed profiles (CPU): `roofline.traffic` comes from the PMC summary
of the kernel, and only while the kernel's sources are what they were when the counters were collected."""
import hashlib
import json
import os


def test_roofline_traffic_is_withheld_when_the_kernel_sources_changed(tmp_path, monkeypatch):
    import bench
    repo = tmp_path
    (repo / "profiles").mkdir()
    (repo / "k").mkdir()
    src = repo / "k" / "kernel.hip"
    src.write_text("__global__ void k() {}\n")
    sha = hashlib.sha256(src.read_bytes()).hexdigest()[:16]
    (repo / "profiles" / "pmc.json").write_text(json.dumps({"hbm_bytes_per_launch": 123, "kernel_sources": {"k/kernel.hip": sha}}))
    (repo / "profiles" / "old.json").write_text(json.dumps({"hbm_bytes_per_launch": 456}))          # summary of an earlier round
    monkeypatch.setattr(bench, "REPO", str(repo))
    t, note = bench.pmc_traffic_checked("pmc.json")
    assert t == 123 and "hashes checked" in note and bench.pmc_traffic("pmc.json") == 123
    t, note = bench.pmc_traffic_checked("old.json")
    assert t == 456 and "hashes" not in note
    src.write_text("__global__ void k() { /* changed */ }\n")
    t, note = bench.pmc_traffic_checked("pmc.json")
    assert t is None and "STALE" in note and "k/kernel.hip" in note
    t, note = bench.pmc_traffic_checked("missing.json")
    assert t is None and "missing" in note


def test_committed_pmc_summaries_are_either_current_or_reported_stale():
    """The two summaries the default line reads carry the hashes of their kernels' sources: the line then either quotes
    their traffic (sources unchanged) or says why it does not - never a figure of another kernel."""
    import bench
    for f in ("pmc_skinny_gemm_f32.json", "pmc_split_gemm_w16.json"):
        assert json.load(open(os.path.join(bench.REPO, "profiles", f))).get("kernel_sources"), f
        t, note = bench.pmc_traffic_checked(f)
        assert (t and "hashes checked" in note) or (t is None and "STALE" in note), (f, note)


def test_dump_outputs_writes_float_arrays_of_the_last_step(tmp_path):
    """`--dump-outputs DIR`: every numeric result as DIR/<name>.npy in float32 / float64 (integers exact as float64),
    strings / None / private keys left out, an oversized array replaced by a fixed sample, 64 MB in all at most."""
    import numpy as np
    import torch
    import bench
    res = dict(rel_pred=[[0, 1, 5], [2, 3, 7]], rel_score=[1, 1], note="text", _private=torch.ones(3),
               nested=[dict(tokens=torch.tensor([[1, -1]], dtype=torch.int32), logit=torch.ones(2, dtype=torch.bfloat16))])
    arrays = bench.output_arrays(res, "result")
    arrays["big"] = np.arange(bench.DUMP_LIMIT_BYTES // 8 // 4 + 1, dtype=np.float32)
    bench.dump_outputs(arrays, str(tmp_path / "out"))
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(got) == {"result.rel_pred", "result.rel_score", "result.nested.0.tokens", "result.nested.0.logit",
                        "big.sample", "big.sample_index"}
    assert got["result.rel_pred"].dtype == np.float64 and got["result.rel_pred"].tolist() == [[0, 1, 5], [2, 3, 7]]
    assert got["result.nested.0.tokens"].dtype == np.float64 and got["result.nested.0.tokens"].tolist() == [[1, -1]]
    assert got["result.nested.0.logit"].dtype == np.float32
    assert got["big.sample"].size == bench.DUMP_SAMPLE
    assert (got["big.sample"] == got["big.sample_index"]).all()                      # arange: value == position
    bench.dump_outputs(arrays, str(tmp_path / "again"))
    assert (np.load(tmp_path / "again" / "big.sample_index.npy") == got["big.sample_index"]).all()
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")) < bench.DUMP_LIMIT_BYTES


def test_plain_run_options(monkeypatch):
    """A plain command line measures the headline alone; `--full` and `--dump-outputs` are opt-in."""
    import sys
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 1, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dumped_relations_have_a_fixed_shape_and_no_output_is_empty(tmp_path):
    """The caller's rel_pred / rel_score lists become relation_scores [objects, objects, 56]: the same triples, the same
    shape whether an image yields relations or none; an empty array is not written."""
    import numpy as np
    import bench
    res = [dict(rel_pred=[[0, 1, 5], [2, 0, 55]], rel_score=[1, 1]), dict(rel_pred=[], rel_score=[])]
    arrays = bench.output_arrays(bench.dense_relations(res, 3), "result")
    arrays["empty"] = np.zeros((0,), dtype=np.float32)
    bench.dump_outputs(arrays, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["result.0.relation_scores.npy", "result.1.relation_scores.npy"]
    r0, r1 = (np.load(tmp_path / f"result.{i}.relation_scores.npy") for i in (0, 1))
    assert r0.shape == r1.shape == (3, 3, 56) and r0.dtype == np.float32
    assert sorted(map(tuple, np.argwhere(r0).tolist())) == [(0, 1, 5), (2, 0, 55)] and not r1.any()
