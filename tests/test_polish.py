"""One-command polish (CPU plumbing): polish() must write byte for byte what
features.run -> infer writes, on a model trained briefly on the assembly's
own windows so that the votes are not all one class."""

import numpy as np
import pytest
import torch

from roko_amd import features as F
from roko_amd.inference import accumulate_votes, infer
from roko_amd.model import RokoModel
from roko_amd.polish import main as polish_main
from roko_amd.polish import polish
from roko_amd.rkdata import RkwFile

CPU = torch.device("cpu")
QUIET = lambda *a, **k: None  # noqa: E731

# tiny_assembly is deterministic (fixed rng seed), so the model trained on its
# windows is the same for every test: train once per session
_trained = {}


@pytest.fixture
def model(tiny_assembly, tmp_path):
    if "state" not in _trained:
        from roko_amd.datasets import InMemoryTrainDataset

        rkw = str(tmp_path / "train.rkw")
        F.run(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], rkw,
              bam_y=tiny_assembly["truth_bam"], workers=1,
              cfg=F.FeatureConfig(region_size=2000, region_overlap=300),
              log=QUIET)
        ds = InMemoryTrainDataset(rkw)
        torch.manual_seed(0)
        m = RokoModel().train()
        opt = torch.optim.Adam(m.parameters(), lr=4e-3)
        # a few small steps on the CPU autograd path: enough to leave the
        # one-class start, cheap enough for the suite
        for step in range(10):
            idx = torch.arange(step * 8, step * 8 + 8) % len(ds)
            logits = m._forward_torch(ds.x[idx])
            loss = torch.nn.functional.cross_entropy(logits.transpose(1, 2),
                                                     ds.y[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()
        _trained["state"] = {k: v.detach().clone()
                             for k, v in m.state_dict().items()}
    m = RokoModel()
    m.load_state_dict(_trained["state"])
    return m.eval()


def _two_step(case, model, tmp_path, cfg, batch_size=32, device=CPU):
    rkw = str(tmp_path / "infer.rkw")
    F.run(case["draft_fasta"], case["reads_bam"], rkw, workers=1, cfg=cfg,
          log=QUIET)
    fasta = str(tmp_path / "two_step.fasta")
    out = infer(rkw, None, fasta, batch_size=batch_size, device=device,
                model=model, log=QUIET)
    return rkw, fasta, out


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def _majority_classes(rkw_path, model):
    """Distinct majority classes of the host vote table of this file."""
    rkw = RkwFile(rkw_path)
    pos, preds = [], []
    with torch.no_grad():
        for gi in range(len(rkw.groups)):
            _, p, x, _ = rkw.group_arrays(gi)
            pos.append(np.array(p))
            preds.append(model(torch.from_numpy(np.array(x)).long())
                         .argmax(dim=2).numpy())
    _, counts = accumulate_votes(np.concatenate(pos), np.concatenate(preds))
    return set(counts.argmax(axis=1).tolist())


@pytest.mark.parametrize("regions", [None, (1500, 300)],
                         ids=["one_region", "overlapping_regions"])
def test_polish_equals_features_then_infer(tiny_assembly, model, tmp_path,
                                           regions):
    cfg = (F.FeatureConfig(seed=5) if regions is None else
           F.FeatureConfig(region_size=regions[0], region_overlap=regions[1],
                           seed=5))
    rkw, want_fasta, want = _two_step(tiny_assembly, model, tmp_path, cfg)
    if regions is not None:
        assert len(RkwFile(rkw).groups) >= 3  # overlaps really exercised
    # the comparison shows nothing if every column votes for one class
    assert len(_majority_classes(rkw, model)) >= 3

    got_fasta = str(tmp_path / "polished.fasta")
    got = polish(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"],
                 None, got_fasta, workers=1, batch_size=32, cfg=cfg,
                 device=CPU, model=model, log=QUIET)
    assert got == want
    assert got["ctg1"] != tiny_assembly["draft"]  # something was polished
    assert _read(got_fasta) == _read(want_fasta)


def test_contig_without_reads_comes_out_as_draft(tiny_assembly, model, rng,
                                                 tmp_path):
    from roko_amd.io.bamio import write_bam
    from roko_amd.io.fasta import write_fasta

    es = tiny_assembly["edit_script"]
    truth = tiny_assembly["truth"]
    bare = "".join(rng.choice(list("ACGT"), 700))
    draft_fasta = str(tmp_path / "two.fasta")
    write_fasta(draft_fasta, [("ctg1", es.draft), ("ctg2", bare)])
    reads = []
    for i in range(150):
        s = int(rng.integers(0, len(truth) - 400))
        rec = es.align_substring(f"r{i}", s, s + 400, flag=16 if i % 2 else 0)
        if rec is not None:
            reads.append(rec)
    reads.sort(key=lambda r: (r.tid, r.pos))
    bam = str(tmp_path / "two.bam")
    write_bam(bam, [("ctg1", len(es.draft)), ("ctg2", len(bare))], reads)
    case = {"draft_fasta": draft_fasta, "reads_bam": bam}

    cfg = F.FeatureConfig(region_size=1500, region_overlap=300, seed=2)
    _, want_fasta, want = _two_step(case, model, tmp_path, cfg)
    got_fasta = str(tmp_path / "polished.fasta")
    got = polish(draft_fasta, bam, None, got_fasta, workers=1, batch_size=32,
                 cfg=cfg, device=CPU, model=model, log=QUIET)
    assert got["ctg2"] == bare
    assert got["ctg1"] != es.draft
    assert got == want
    assert _read(got_fasta) == _read(want_fasta)


def test_cli_writes_the_same_file(tiny_assembly, model, tmp_path):
    """`python -m roko_amd.polish` entry with worker processes. Both sides
    pick their device themselves, so the files match with or without a GPU."""
    ckpt = str(tmp_path / "m.pth")
    torch.save(model.state_dict(), ckpt)
    rkw = str(tmp_path / "infer.rkw")
    F.run(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], rkw,
          workers=1, cfg=F.FeatureConfig(seed=3), log=QUIET)
    want_fasta = str(tmp_path / "two_step.fasta")
    infer(rkw, ckpt, want_fasta, batch_size=32, log=QUIET)

    got_fasta = str(tmp_path / "cli.fasta")
    polish_main([tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"],
                 ckpt, got_fasta, "--t", "2", "--b", "32", "--seed", "3"])
    assert _read(got_fasta) == _read(want_fasta)


def test_device_votes_need_a_gpu(tiny_assembly, model, tmp_path):
    rkw = str(tmp_path / "infer.rkw")
    F.run(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], rkw,
          workers=1, log=QUIET)
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        infer(rkw, None, None, device=CPU, model=model, log=QUIET,
              votes="device")
    with pytest.raises(ValueError, match="votes must be"):
        infer(rkw, None, None, device=CPU, model=model, log=QUIET,
              votes="gpu")


def test_device_votes_are_single_process(tiny_assembly, model, tmp_path,
                                         monkeypatch):
    import roko_amd.inference as inference

    rkw = str(tmp_path / "infer.rkw")
    F.run(tiny_assembly["draft_fasta"], tiny_assembly["reads_bam"], rkw,
          workers=1, log=QUIET)
    monkeypatch.setattr(inference, "init_distributed", lambda: (0, 0, 2))
    with pytest.raises(ValueError, match="single-process"):
        infer(rkw, None, None, device=CPU, model=model, log=QUIET,
              votes="device")
