"""Full-stack integration: train pipeline -> artifacts -> embedding REST
server (in-process) -> repo-specific model over HTTP contract -> predictor
routing -> worker applies labels from a queued event. The whole L1-L5
production path (SURVEY.md §1 data-flow) with only the GitHub REST calls
faked."""
import pytest
import torch

from code_intelligence_amd.engine.inference import InferenceWrapper
from code_intelligence_amd.gh import bigquery
from code_intelligence_amd.gh.gcs_util import ObjectStore
from code_intelligence_amd.label.issue_label_predictor import IssueLabelPredictor
from code_intelligence_amd.label.queueing import LocalQueue
from code_intelligence_amd.label.repo_specific_model import RepoSpecificLabelModel
from code_intelligence_amd.label.trainers import run_training_pipeline
from code_intelligence_amd.label.worker import Worker
from code_intelligence_amd.models.awd_lstm import AWDLSTM
from code_intelligence_amd.serve.app import create_app
from code_intelligence_amd.text.tokenizer import Vocab, defaults_specials


class FlaskSession:
    """requests-like session backed by the flask test client (the worker's
    HTTP boundary to the embedding server)."""

    def __init__(self, client):
        self.client = client

    def post(self, url, json=None, **kw):
        path = "/" + url.split("/", 3)[-1] if "://" in url else url
        r = self.client.post(path, json=json)

        class R:
            status_code = r.status_code
            content = r.data
        return R()


class RecordingGitHub:
    def __init__(self):
        self.labels = []
        self.comments = []

    def add_labels(self, o, r, n, labels):
        self.labels.append(labels)

    def add_comment(self, o, r, n, body):
        self.comments.append(body)

    def list_comments(self, o, r, n):
        return []


@pytest.mark.parametrize("qrnn", [False, True], ids=["lstm", "qrnn"])
def test_full_production_path(tmp_path, qrnn):
    torch.manual_seed(0)
    words = [f"w{i}" for i in range(300)]
    vocab = Vocab(defaults_specials + words)
    model = AWDLSTM(vocab_sz=len(vocab), emb_sz=16, n_hid=24, n_layers=2,
                    qrnn=qrnn)
    wrapper = InferenceWrapper(encoder=model.encoder, vocab=vocab, device="cpu")

    # archive with a linearly-separable label structure
    events = []
    for i in range(90):
        label = "bug" if i % 2 == 0 else "feature"
        word = "crash" if label == "bug" else "request"
        events.append({"org": "o", "repo": "r", "issue_num": i,
                       "title": f"{word} w{i % 20}", "body": f"{word} body",
                       "labels": [label],
                       "updated_at": "2024-01-01T00:00:00Z"})
    bigquery.write_archive_events(events, tmp_path / "arch" / "s.jsonl")
    store = ObjectStore(root=tmp_path / "store")

    # L2: training pipeline publishes artifacts
    result = run_training_pipeline("o", "r", wrapper, store=store,
                                   archive_root=tmp_path / "arch")
    assert set(result["labels"]) == {"bug", "feature"}

    # L3: embedding REST server (in-process flask)
    app = create_app(wrapper=wrapper)
    session = FlaskSession(app.test_client())

    # L4: repo model loads artifacts, predictor routes to it
    repo_model = RepoSpecificLabelModel.from_repo("o", "r", store=store,
                                                  session=session)
    predictor = IssueLabelPredictor(model_config={}, universal=repo_model)

    # L4/L5: worker consumes a queued event and applies labels
    gh = RecordingGitHub()
    q = LocalQueue()
    issue = {"title": "crash w2", "comments": ["crash body"],
             "labels": [], "removed_labels": []}
    w = Worker(queue=q, predictor=predictor, github=gh,
               repo_config_fn=lambda o, r: None)
    preds = predictor.predict_labels_for_data("o", "r", issue["title"],
                                              issue["comments"])
    added = w.add_labels_to_issue("o", "r", 2, preds, issue_data=issue)
    # threshold search on tiny data may abstain; the contract under test is
    # that the path runs end-to-end and anything applied is a known label
    for l in added:
        assert l in {"bug", "feature"}
    if added:
        assert gh.labels and gh.comments


@pytest.mark.timeout(180)
def test_bench_contract_cpu_fallback():
    """bench.py must emit exactly one driver-contract JSON line on stdout
    (CPU fallback config) — the fields the round driver parses."""
    import json
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    r = subprocess.run([sys.executable, str(root / "bench.py"),
                        "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
              "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config"):
        assert k in out, k
    assert out["metric"] == "LM tokens/sec (whole node)"
    assert out["scaling"] == "weak" and out["data"] == "synthetic"
    assert out["value"] > 0 and out["n_gpus"] == 1
    assert {"model", "global_batch", "seq_len", "parallelism"} <= set(out["config"])


@pytest.mark.timeout(300)
def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's results as float .npy
    files that are identical from run to run; a plain run carries no serve
    object, --full does, and --full leaves the timed path's results alone."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    import numpy as np
    root = Path(__file__).resolve().parents[1]

    # the options are host-side plumbing: hide any GPU from the child so the
    # small CPU config runs everywhere and the results compare exactly
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")

    def run(out_dir, *extra):
        r = subprocess.run([sys.executable, str(root / "bench.py"),
                            "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--dump-outputs", str(out_dir), *extra],
                           capture_output=True, text=True, timeout=140,
                           env=env)
        assert r.returncode == 0, r.stderr[-800:]
        lines = [l for l in r.stdout.strip().splitlines()
                 if l.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])

    plain = run(tmp_path / "a")
    full = run(tmp_path / "b", "--full")
    assert "serve" not in plain and "serve" in full
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0
    files = sorted(p.name for p in (tmp_path / "a").glob("*.npy"))
    assert "loss.npy" in files
    assert any(f.startswith("param.") for f in files)
    assert any(f.startswith("hidden.") for f in files)
    assert files == sorted(p.name for p in (tmp_path / "b").glob("*.npy"))
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64), (f, a.dtype)
        assert np.isfinite(a).all(), f
        assert np.array_equal(a, b), f
        total += a.nbytes
    assert total <= 64 * 2 ** 20


@pytest.mark.timeout(420)
def test_bench_world8_torchrun_cpu():
    """Launch bench.py EXACTLY like the driver's 8-GPU scale run
    (torch.distributed.run, --nproc-per-node 8) but on CPU/gloo: proves
    the rendezvous, env parsing, DDP bucketer world-8 wiring and the
    rank-0-only JSON contract without a GPU node."""
    import json
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
         "--master-port", "29771", str(root / "bench.py"),
         "--gpus", "8", "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=390)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-1200:])
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]  # rank 0 only
    out = json.loads(lines[0])
    assert out["config"]["parallelism"] == "dp8"
    assert out["config"]["global_batch"] == 2 * 8  # CPU-fallback bs=2
    assert out["value"] > 0
