"""The lazy-L2 SGD step in two launches (k_fwd_bwd, k_finalize_update; include/tlsan.h, tlsan_train_step): the finalize's
workgroups store the dense parameters and commit the table scale, and a clipped step's correction runs at the head of the
next step's fused kernel -- or in tlsan_state_flush when something else reads the parameters first.

Shapes: d = 64 and d = 128; B = 32 (a fused-kernel grid smaller than the 64 correcting workgroups), B = 1024 and B = 2048
(larger, both workgroup geometries of d = 128).  The category counts keep every category in one workgroup (400 categories at
the large batches: fewer than 96 uses each), since shapes with shared categories keep the commit launch.
Tolerances: those of the lazy train-step tests of tests/test_gpu_parity.py (loss 2e-4, global norm 3e-4, parameters 5e-4 of
the tensor's largest magnitude after several steps), against the fp64 oracle; the three-launch form (TLSAN_TWO_LAUNCH=0, read
once per process, hence the child process) must agree BIT FOR BIT on unclipped steps."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import tlsan_oracle as orc
from tests.helpers import batch_tuple, make_config, model, p32, random_batch, random_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 32), (64, 1024), (64, 2048), (128, 32), (128, 1024), (128, 2048)]
STEPS = 8
CLIPPED = (2, 3, 5, 7)     # (0-based: the third and the sixth step, two in a row, and the last one)
LR, REG = 0.9, 2e-2        # (test_lazy_l2_matches_dense_oracle's: the decay is visible in the scale)
NO_CLIP, CLIP = 1e6, 0.02


def _problem(d, B):
    big = B > 32
    cfg = make_config(U=3000 if big else 300, I=2000 if big else 200, C=400 if big else 9, d=d,
                      max_gradient_norm=NO_CLIP, regulation_rate=REG)
    p = p32(random_params(cfg, seed=7 * d + B))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=B, Sn=1 + s % 3, seed=900 + 13 * s + B)[0] for s in range(STEPS)]
    return cfg, p, cat, batches


def _model(cfg, cat, p):       # (helpers.model with this file's two constants: the lazy-L2 step, and a copy of cfg for the model)
    return model(dict(cfg), cat, p, l2_mode="lazy")


def _run(m, batches, clips, ahead):
    """The steps, each with its own clip norm; ahead: the index of the next two batches is built while a step runs, so a step
    starts with the fused kernel (and makes a clipped predecessor's correction at its head).  -> losses, global norms"""
    dbs = [m.device_batch(batch_tuple(b)) for b in batches]
    losses, norms = [], []
    for t, db in enumerate(dbs):
        m.config["max_gradient_norm"] = clips[t]
        if ahead:
            m.train_async(db, LR, next_batch=dbs[t + 1] if t + 1 < len(dbs) else None,
                          after_next=dbs[t + 2] if t + 2 < len(dbs) else None)
        else:
            m.train_async(db, LR)
        o = m._out.cpu().numpy()       # (the step's outputs: not one of the tensors whose read flushes)
        losses.append(float(o[0]))
        norms.append(float(o[1]))
    return losses, norms


def unclipped_digest(d, B):
    """sha256 over every loss, global norm and parameter (stored tables, scale, dense weights, then the folded parameters)
    of eight unclipped steps with the index built ahead"""
    import torch
    cfg, p, cat, batches = _problem(d, B)
    m = _model(cfg, cat, p)
    losses, norms = _run(m, batches, [NO_CLIP] * STEPS, ahead=True)
    h = hashlib.sha256()
    h.update(np.asarray(losses + norms, np.float64).tobytes())
    for k in ("item_emb", "item_b", "user_emb", "usert_emb", "cate_emb", "dense"):
        h.update(getattr(m, k).float().cpu().numpy().tobytes())
    h.update(np.float32(m.table_scale()).tobytes())
    got = m.get_params()
    for k in sorted(got):
        h.update(np.ascontiguousarray(got[k]).tobytes())
    torch.cuda.synchronize()
    return h.hexdigest()


_CHILD = """
import json, sys
sys.path.insert(0, %r)
from tests.test_gpu_two_launch import SHAPES, unclipped_digest
print("DIGESTS " + json.dumps({"%%d,%%d" %% s: unclipped_digest(*s) for s in SHAPES}))
"""


@pytest.fixture(scope="module")
def three_launch_digests():
    env = dict(os.environ, TLSAN_TWO_LAUNCH="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("DIGESTS ")][-1]
    return json.loads(line[len("DIGESTS "):])


@pytest.mark.parametrize("d,B", SHAPES)
def test_unclipped_steps_leave_the_three_launch_bits(d, B, three_launch_digests):
    assert os.environ.get("TLSAN_TWO_LAUNCH", "1") != "0"
    assert unclipped_digest(d, B) == three_launch_digests["%d,%d" % (d, B)]


_ORACLE = {}


def _oracle(d, B):
    """the mixed sequence in the fp64 oracle, once per shape: per-step loss and norm, the final parameters"""
    if (d, B) not in _ORACLE:
        cfg, p, cat, batches = _problem(d, B)
        q, out = dict(p), []
        for t, b in enumerate(batches):
            clip = CLIP if t in CLIPPED else NO_CLIP
            lo, q, info = orc.train_step(q, cat, b, 8, REG, lr=LR, clip=clip)
            out.append((lo, info["norm"]))
        _ORACLE[(d, B)] = (out, q)
    return _ORACLE[(d, B)]


@pytest.mark.parametrize("ahead", [True, False])
@pytest.mark.parametrize("d,B", SHAPES)
def test_clipped_steps_match_the_oracle(d, B, ahead):
    """Clipped steps among unclipped ones, two in a row and a clipped LAST step, read back through the plain attributes and
    through get_params; ahead = False: every step builds its index itself, so the library flushes before it."""
    cfg, p, cat, batches = _problem(d, B)
    ref, q = _oracle(d, B)
    clips = [CLIP if t in CLIPPED else NO_CLIP for t in range(STEPS)]
    runs = []
    for rep in range(2):
        m = _model(cfg, cat, p)
        losses, norms = _run(m, batches, clips, ahead)
        for t, (lo, no) in enumerate(ref):
            print("step %d loss %.7g (oracle %.7g) norm %.7g (oracle %.7g)" % (t, losses[t], lo, norms[t], no))
            assert abs(losses[t] - lo) < 2e-4 * max(1.0, abs(lo)), t
            assert abs(norms[t] - no) < 3e-4 * no, t
            assert t not in CLIPPED or no > CLIP     # (those steps ARE clipped)
        # the plain attributes after the clipped last step: stored tables times the scale, the dense weights
        P = m.table_scale()
        flat = m.pack_dense({k: np.asarray(v, np.float32) for k, v in q.items()})
        dn = m.dense.cpu().numpy().astype(np.float64)
        assert np.abs(dn - flat).max() < 5e-4 * np.abs(flat).max() + 1e-6
        for k in ("item_emb", "user_emb", "cate_emb", "usert_emb"):
            g = getattr(m, k).float().cpu().numpy().astype(np.float64) * P
            assert np.abs(g - q[k]).max() < 5e-4 * np.abs(q[k]).max() + 1e-6, k
        got = m.get_params()
        for k in q:
            g = np.asarray(got[k], np.float64).reshape(q[k].shape)
            assert np.abs(g - q[k]).max() < 5e-4 * np.abs(q[k]).max() + 1e-6, k
        runs.append((losses, norms, got))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for k in runs[0][2]:
        assert np.array_equal(runs[0][2][k], runs[1][2][k]), k


@pytest.mark.parametrize("ahead", [True, False])
@pytest.mark.parametrize("d", [64, 128])
def test_planted_nonfinite_row_poisons_this_step_and_the_next(d, ahead):
    """test_nonfinite_inputs_give_nonfinite_loss's plants (a NaN and a +Inf in a gathered item row, a gathered user row):
    the step's loss is non-finite, and so is the next step's -- the NaN coefficient takes the correcting pass."""
    cfg = make_config(U=30, I=50, C=7, d=d, Ls=10)
    p0 = p32(random_params(cfg, seed=5 * d + 10))
    b, cat = random_batch(cfg, B=40, Sn=3, seed=d + 1)
    it, us = int(b["hist_i"][0, 0]), int(b["u"][3])
    for key, idx in (("item_emb", (it, 5)), ("user_emb", (us, 2))):
        for bad in (np.nan, np.inf):
            p = {k: v.copy() for k, v in p0.items()}
            p[key][idx] = bad
            m = _model(cfg, cat, p)
            losses, norms = _run(m, [b, b], [5.0, 5.0], ahead)
            assert not np.isfinite(losses[0]) and not np.isfinite(losses[1]), (key, bad, losses)
            assert not np.isfinite(norms[0]), (key, bad, norms)
    m = _model(cfg, cat, p0)
    losses, _ = _run(m, [b, b], [5.0, 5.0], ahead)
    assert np.isfinite(losses).all()


def test_graph_replays_of_a_clipped_step_equal_eager():
    cfg = make_config(U=200, I=150, C=9, d=128, max_gradient_norm=CLIP, regulation_rate=REG)
    p = p32(random_params(cfg, seed=71))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=64, Sn=3, seed=400 + s)[0] for s in range(3)]
    outs = []
    for mode in ("eager", "graph"):
        m = _model(cfg, cat, p)
        if mode == "graph":
            graphs = [m.capture_step(batch_tuple(b), 0.7) for b in batches]
            m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})   # (capture_step ran a warm step per batch)
            for rep in range(2):
                for g in graphs:
                    m.replay(g)
        else:
            for rep in range(2):
                for b in batches:
                    m.train_async(batch_tuple(b), 0.7)
        assert m.last_gnorm() > CLIP       # (the steps are clipped)
        outs.append(m.get_params())
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_evaluation_directly_after_a_clipped_step():
    import torch
    cfg = make_config(U=300, I=200, C=9, d=128, max_gradient_norm=CLIP, regulation_rate=REG)
    p = p32(random_params(cfg, seed=51))
    b, cat = random_batch(cfg, B=24, Sn=2, seed=300)
    tb, _ = random_batch(cfg, B=200, Sn=2, seed=99, test=True)
    _, q, info = orc.train_step(dict(p), cat, b, 8, REG, lr=LR, clip=CLIP)
    assert info["norm"] > CLIP
    res = []
    for explicit in (False, True):
        m = _model(cfg, cat, p)
        m.train_async(batch_tuple(b), LR)
        if explicit:
            m._flush()
            torch.cuda.synchronize()
        auc = m.eval_auc(None, batch_tuple(tb, True))
        li, lj, _, _ = m.forward(batch_tuple(tb, True), is_test=True)
        res.append((auc, li.cpu().numpy(), lj.cpu().numpy()))
    assert res[0][0] == res[1][0]
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    ref = orc.forward(q, cat, tb, 8)
    assert np.abs(res[0][1] - ref["logits"]).max() < 3e-4
