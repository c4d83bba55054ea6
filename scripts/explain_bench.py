#!/usr/bin/env python3
"""Cost of explaining a recommendation list (Model.explain) at the bench shape: the Electronics-scale tables (d = 128),
B = 4096, Kc = 10 listed items per row, top = 3, by="item".  Timed, all on the same batch:

    forward(want_att)            what explain runs first (the attention weights)
    recommend(batch, 10)         the yardstick: the list that is being explained
    explain, top only            Model.explain(parts=False)
    explain, parts and top       Model.explain(parts=True)
    tlsan_explain alone          the library call on attention weights already there, both forms
    torch decomposition          the same parts as gathers + einsum on the device (the host-side alternative), checked
                                 against the kernel's parts before it is timed

Without --part this is a list of steps for scripts/steps.py (fresh processes, each under its own time limit, nothing more
after the first that fails; logs under --out) and prints the medians.  Times are host clocks around a synchronised loop of
--iters calls behind a warm-up.  --d 256: the same with hidden_units = 256.

    python scripts/explain_bench.py [--rounds 3] [--out measure_out/explain]
    python scripts/explain_bench.py --part 1"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

B, KC, TOP = 4096, 10, 3


def torch_parts(m, db, items, att0, att1):
    """The decomposition of include/tlsan.h (tlsan_explain) as torch expressions -> parts [B, Kc, R]."""
    import torch
    d, H = m.config["hidden_units"], m.config["num_heads"]
    dh, Bn = d // H, db.B
    P = m.state[:4].view(torch.float32)
    chan = lambda a: a.view(H, Bn, -1, dh).permute(1, 2, 0, 3).reshape(Bn, -1, d)
    a0, a1 = chan(att0), chan(att1)
    emb = lambda ids: torch.cat([m.item_emb[ids].float(), m.cate_emb[m.item_cate[ids].long()].float()], -1) * P
    g = items.clamp(min=0).long()
    w = emb(g)
    K, k0, gamma = m.dense[m.lay.K:m.lay.K + d * d].view(d, d), m.dense[m.lay.k0:m.lay.k0 + d], m.dense[m.lay.gamma]
    u = db.u.long()
    u_emb = torch.cat([m.user_emb[u].float(), m.cate_emb[db.u_cate.long()].float()], -1) * P
    x = a1[:, 0].unsqueeze(1) * w
    v = x @ K.t()
    ah = a0 * emb(db.hist_i.long()) * (gamma * (m.usert_emb[u] * P) * db.hist_t).unsqueeze(-1)
    cols = [m.item_b[g].unsqueeze(-1), (u_emb.unsqueeze(1) * w).sum(-1, keepdim=True), (x * k0).sum(-1, keepdim=True),
            torch.einsum("blc,bkc->bkl", ah, v) * (torch.arange(ah.shape[1], device=w.device) < db.sl[:, None]).unsqueeze(1)]
    if db.Sn:
        an = a1[:, 1:] * emb(db.hist_i_new.long())
        cols.append(torch.einsum("bjc,bkc->bkj", an, w) * (torch.arange(db.Sn, device=w.device) < db.sl_new[:, None]).unsqueeze(1))
    return torch.cat(cols, -1) * (items >= 0).unsqueeze(-1)


def part(n, d):
    from catidx_bench import timed
    from tlsan_amd import _lib as L
    from tlsan_amd import synth
    from tlsan_amd.model import Model, explain
    over = {} if d == 128 else dict(hidden_units=d, itemid_embedding_size=d // 2, userid_embedding_size=d // 2, cateid_embedding_size=d // 2)
    cfg = synth.make_config("electronics", **over)
    m = Model(cfg, synth.item_cate_list(cfg), l2_mode="lazy", init="device")
    db = m.device_batch(synth.make_batches(cfg, 1, B, seed=9, test=True)[0], is_test=True)
    out = lambda case, ms, **kw: print(json.dumps(dict(part="explain", d=d, case=case, ms=round(ms, 4), **kw)), flush=True)
    out("forward(want_att)", timed(lambda: m.forward(db, is_test=True, want_att=True), n))
    out("recommend(batch, %d)" % KC, timed(lambda: m.recommend(db, KC), n))
    ids = m.recommend(db, KC)[0]
    out("explain, top only", timed(lambda: m.explain(db, ids, top=TOP), n))
    out("explain, parts and top", timed(lambda: m.explain(db, ids, top=TOP, parts=True), n))
    m.forward(db, is_test=True, want_att=True)
    a0, a1, st = m.att0, m.att1, m._stream()
    call = lambda parts: explain(m.lib, m.dims, m.cparams, db, a0, a1, ids, TOP, L.EXPLAIN_BY_ITEM, L.EXPLAIN_POSITIVE, parts, st)
    out("tlsan_explain alone, top only", timed(lambda: call(False), n))
    out("tlsan_explain alone, parts and top", timed(lambda: call(True), n))
    got, ref = call(True).parts, torch_parts(m, db, ids, a0, a1)
    diff = float((got - ref).abs().max())
    if not diff < 1e-4:
        raise SystemExit("the torch decomposition and the kernel disagree: max |diff| = %g" % diff)
    out("torch decomposition (parts only)", timed(lambda: torch_parts(m, db, ids, a0, a1), n), max_diff=diff)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", type=int, default=0)
    ap.add_argument("--d", type=int, default=128, choices=(128, 256))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("measure_out", "explain"))
    a = ap.parse_args()
    if a.part:
        return part(a.iters, a.d)
    from shelves_bench import lines_of
    from steps import log_path, run_steps
    me = [sys.executable, os.path.abspath(__file__), "--part", 1, "--iters", a.iters, "--d", a.d]
    rc = run_steps([("explain_d%d_%d" % (a.d, r), me, {}, 300, ROOT) for r in range(a.rounds)], a.out)
    if rc:
        return rc
    rows = {}
    for r in range(a.rounds):
        for row in lines_of(log_path(a.out, "explain_d%d_%d" % (a.d, r)), '"part"'):
            rows.setdefault(row["case"], []).append(row["ms"])
    print("d = %d, B = %d, Kc = %d, top = %d, by item; ms: median (min max of %d processes)" % (a.d, B, KC, TOP, a.rounds))
    for case, v in rows.items():
        v = sorted(v)
        print("%-40s %9.4f   (%.4f %.4f)" % (case, v[len(v) // 2], v[0], v[-1]))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
