"""Driver: counterpart of the reference's ``TLSAN/train.py`` (flags :26-54, loop :121-249).

    python -m tlsan_amd.train --dataset tests/golden/packed_clothing.npz [--flag=value ...]

Same flag names and defaults as the reference (``tf.app.flags`` -> argparse), same flow:
initial AUC / P@k / R@k, ``max_epochs`` epochs of shuffled batches, evaluation every
``eval_freq`` steps, learning rate 1.0 -> 0.1 at step 150000, save when the test AUC improves
(> 0.8).  ``--dataset`` takes either a ``dataset.pkl`` written by the reference's
``build_dataset.py`` (train.py:131-135) or a ``packed_<name>.npz`` export (tests/golden/).
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import pickle
import random
import re
import shutil
import time

import numpy as np
import torch

from .input import DataInput, DataInputTest, PackedSet, item_self_information, load_packed
from .model import (KS, LAZY_ADAGRAD_OPTIMIZERS, ListMetricCounters, ListMetrics, Model, SeenItems, full_ranking_metrics,
                    hits_and_rows, metrics_from_histogram)

FLAGS = [  # (name, type, default)  -- train.py:26-54
    ("hidden_units", int, 64), ("num_blocks", int, 1), ("num_heads", int, 8), ("Ls", int, 10),
    ("dropout", float, 0.0), ("regulation_rate", float, 0.00005),
    ("itemid_embedding_size", int, 32), ("userid_embedding_size", int, 32), ("cateid_embedding_size", int, 32),
    ("model_dir", str, "save_path"), ("optimizer", str, "sgd"), ("learning_rate", float, 1.0),
    ("max_gradient_norm", float, 5.0), ("train_batch_size", int, 32), ("test_batch_size", int, 128),
    ("max_epochs", int, 20), ("display_freq", int, 100), ("eval_freq", int, 1000),
]


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name, typ, default in FLAGS:
        ap.add_argument("--" + name, type=typ, default=default)
    ap.add_argument("--from_scratch", type=lambda s: s.lower() != "false", default=True)
    ap.add_argument("--dataset", default=None, help="dataset.pkl of the reference's build_dataset.py, or a packed_<name>.npz export")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--max_steps", type=int, default=0, help="stop early (0 = run max_epochs)")
    ap.add_argument("--norm_mode", default="tf18", choices=["tf18", "dedup"])
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--table_dtype", default="f32", choices=["f32", "bf16"],
                    help="storage of item/user/category tables (bf16: fp32 arithmetic, stochastic rounding on update)")
    ap.add_argument("--wire_dtype", default="f32", choices=["f32", "bf16"],
                    help="sharded driver with --static_rows: embedding values of the rows that cross the wire (owners keep fp32)")
    ap.add_argument("--static_rows", type=int, default=0,
                    help="sharded driver, lazy L2: 0 = exchange sizes follow the batch (read by the host once a step); "
                         "1 = fixed-size exchanges sized from the first batch (x1.5); N > 1 = N row slots per rank pair. "
                         "A batch that does not fit raises at the next check (every 1024 steps, at evaluation, at the end)")
    ap.add_argument("--matrix_dtype", default="f32", choices=["f32", "bf16"],
                    help="arithmetic of the fused kernel's matrix products (bf16: operands rounded to bfloat16, fp32 accumulate)")
    ap.add_argument("--l2_mode", default="dense", choices=["dense", "lazy"])
    ap.add_argument("--eval_topk", type=int, default=1,
                    help="P@k / R@k at every evaluation point like the reference (train.py:209-218); 0: once at the end")
    ap.add_argument("--sharded", type=int, default=0,
                    help="1: row-sharded tables over the ranks of torch.distributed (implied by WORLD_SIZE > 1)")
    ap.add_argument("--seed", type=int, default=1234,
                    help="seed of the variables' initial values (the reference seeds everything with 1234, train.py:15-17; "
                         "TensorFlow's own stream cannot be reproduced, so this picks ONE draw of the same distributions)")
    ap.add_argument("--shuffle_seed", type=int, default=1234, help="seed of the epoch shuffle stream (train.py:15,191: 1234)")
    ap.add_argument("--device_input", type=int, default=1,
                    help="1: keep the sample sets in HBM and assemble batches on the device (tlsan_amd.device_input); "
                         "0: the host batcher (tlsan_amd.input), one upload per batch")
    ap.add_argument("--recommend_k", type=int, default=0,
                    help="at the end of training, write <model_dir>/recommend_top<K>.npz: the K best items over all items "
                         "for every test row (arrays user, ids, scores); 0 = off")
    ap.add_argument("--recommend_exclude", default="history", choices=["history", "none", "seen"],
                    help="items kept out of the recommendations: 'history' = the items the test row's input holds (its "
                         "last Ls items and its current session -- what the batch carries), 'none' = nothing, 'seen' = "
                         "every item of the user's training samples and the row's input")
    ap.add_argument("--recommend_pages", type=int, default=1, metavar="P",
                    help="with --recommend_k: lists of P x K entries -- P pages of K chained through list cursors "
                         "(Model.recommend_deep: one forward, one scan a page, the exact ranking at any depth); the file is "
                         "recommend_top<P x K>.npz.  It goes without the diversity flags, --shortlist_index, --recommend_metrics "
                         "and --recommend_explain")
    ap.add_argument("--recommend_diversity", type=float, default=0.0,
                    help="with --recommend_k: re-rank each row's pool by maximal marginal relevance, theta in [0, 1] "
                         "(0 = relevance only, 1 = novelty only after the first pick; Model.recommend's diversity)")
    ap.add_argument("--recommend_per_category", type=int, default=0,
                    help="with --recommend_k: at most this many items of one category in a row's list (0 = no cap)")
    ap.add_argument("--recommend_pool", type=int, default=0,
                    help="with --recommend_diversity / --recommend_per_category: the best N items per row the list is picked "
                         "from, recommend_k <= N <= 256 (0 = min(256, max(4 K, 32)))")
    ap.add_argument("--recommend_metrics", type=int, default=0, choices=[0, 1],
                    help="with --recommend_k: 1 = measure the lists over the whole test set (Model.list_metrics: ILD, categories, "
                         "the largest per-category count, HR / NDCG / MRR of the test positives, novelty by the training "
                         "set's self-information, catalogue coverage and the Gini coefficient of the exposure), print them "
                         "and write <model_dir>/recommend_top<K>_metrics.json")
    ap.add_argument("--recommend_boost", default="", metavar="PATH.npy",
                    help="with --recommend_k: a per-item score adjustment, fp32 [item_count] (np.save): every score becomes "
                         "score + boost[item] inside the selection (Model.recommend's boost=).  -inf buries an item, it does "
                         "not remove it")
    ap.add_argument("--recommend_novelty", type=float, default=0.0, metavar="ALPHA",
                    help="with --recommend_k: boost = ALPHA x the items' self-information over the training set "
                         "(input.item_self_information, the novelty weight of --recommend_metrics): ALPHA > 0 pays for rare "
                         "items, ALPHA < 0 for popular ones.  Summed with --recommend_boost when both are given; with "
                         "--recommend_metrics 1 the metrics are those of the lists as served")
    ap.add_argument("--recommend_categories", default="",
                    help="with --recommend_k: recommend within the items of these categories only, e.g. 3,7,12 (an ItemScope: "
                         "only those items are scored)")
    ap.add_argument("--recommend_same_category", type=int, default=0, choices=[0, 1],
                    help="with --recommend_k: 1 = each row's list holds items of the category of the last item of the row's "
                         "input only (last_item_categories)")
    ap.add_argument("--similar_k", type=int, default=0,
                    help="at the end of training, write <model_dir>/similar-<K>.npz: the K nearest items of every item "
                         "(item [I], ids [I, K], scores [I, K]; 0 = off)")
    ap.add_argument("--similar_metric", default="cosine", choices=["cosine", "dot"],
                    help="the similarity of --similar_k: cosine, or the dot product of the item vectors")
    ap.add_argument("--similar_same_category", type=int, default=0, choices=[0, 1],
                    help="with --similar_k: 1 = an item's list holds items of its own category only")
    ap.add_argument("--category_index", type=int, default=0, choices=[0, 1],
                    help="1 = build a per-category item index (Model.category_index; over the items of --recommend_categories "
                         "when given) and pass it wherever --recommend_same_category / --similar_same_category apply: a row "
                         "scores its category's items only.  The files written are the same")
    ap.add_argument("--recommend_explain", type=int, default=0, metavar="R",
                    help="with --recommend_k: the R strongest history sources of every listed item, 1..16 (Model.explain, by item, "
                         "larger part first): the lists' file gains why_item, why_value and why_kind, each [rows, K, R] (-1 / 0 / "
                         "-1 where a row has fewer sources; kind 0 = the long window, 1 = the session); single GPU")
    ap.add_argument("--shelves", type=int, default=0, metavar="S",
                    help="at the end of training, write <model_dir>/shelves_<S>x<M>.npz: for every test row its S best "
                         "categories and the M best items of each (Model.shelves over the per-category index: users [N], cats "
                         "[N, S], ids [N, S, M], scores [N, S, M]); needs --category_index 1 and --shelf_items; --recommend_exclude "
                         "applies as it does to the lists; 0 = off")
    ap.add_argument("--shelf_items", type=int, default=0, metavar="M",
                    help="with --shelves: items of a shelf, 1..64 with S x M <= 256")
    ap.add_argument("--shelf_min_items", type=int, default=1, metavar="N",
                    help="with --shelves: a category is a shelf only when it has N items left for the row, 1..M")
    ap.add_argument("--shelf_skip_last", type=int, default=0, choices=[0, 1],
                    help="with --shelves: 1 = the category of the last item of a row's input is not offered to that row")
    ap.add_argument("--cluster_index", type=int, default=0, metavar="NLISTS",
                    help="with --recommend_k: build a clustered item index of NLISTS lists (Model.cluster_index: k-means over "
                         "the item vectors; over the items of --recommend_categories when given) and write APPROXIMATE lists: "
                         "each row scores the --cluster_probes lists nearest to it.  With --recommend_metrics 1 the recall@k "
                         "of these lists against the exact ones over the test rows is printed.  0 = off")
    ap.add_argument("--cluster_probes", type=int, default=8, metavar="P",
                    help="with --cluster_index: lists a row probes, 1..64")
    ap.add_argument("--shortlist_index", type=int, default=0, choices=[0, 1],
                    help="with --recommend_k: 1 = serve the lists through a bf16 shortlist index (Model.shortlist_index): the same "
                         "EXACT lists in two stages, rows without a certificate through the full scan; the share of certified "
                         "rows is printed.  Not with a scope, a category or another index")
    ap.add_argument("--shortlist", type=int, default=0, metavar="N",
                    help="with --shortlist_index: entries of a row's shortlist, 16..256 and above the list asked of the first "
                         "stage (0 = min(256, max(4 n, 64)))")
    ap.add_argument("--audience_k", type=int, default=0,
                    help="at the end of training, write <model_dir>/audience-<K>.npz: for every item of --audience_items the K "
                         "best test rows (Model.audience over the user vectors of the test set, one row per user): item [Q], "
                         "users [Q, K], rows [Q, K], scores [Q, K]; 0 = off")
    ap.add_argument("--audience_pages", type=int, default=1, metavar="P",
                    help="with --audience_k: audiences of P x K rows -- P pages of K chained through list cursors "
                         "(Model.audience_deep: one scan a page, any depth); the file is audience-<P x K>.npz; --audience_k itself "
                         "stays 1..256")
    ap.add_argument("--audience_items", default="",
                    help="with --audience_k (required): the global item ids whose audiences are wanted, e.g. 3,7,12")
    ap.add_argument("--audience_exclude", default="none", choices=["none", "seen"],
                    help="with --audience_k: 'seen' = a user whose training samples hold the item stays out of its audience")
    ap.add_argument("--eval_negatives", type=int, default=0,
                    help="sampled evaluation at every evaluation point: rank each test label among N sampled negatives "
                         "and report HR@k, NDCG@k (k = 1, 5, 10, 20), MRR and AUC_N; 0 = off")
    ap.add_argument("--eval_neg_seed", type=int, default=1234,
                    help="seed of the negatives (a test row's negatives depend on the seed and its position in the test set)")
    ap.add_argument("--eval_neg_exclude", default="history", choices=["history", "none", "seen"],
                    help="items never drawn as a row's negatives besides its label: 'history' = the items the test row's "
                         "input holds, 'none' = nothing, 'seen' = every item of the user's training samples and the row's input")
    ap.add_argument("--eval_rank_exclude", default="off", choices=["off", "none", "history", "seen"],
                    help="full-ranking evaluation at every evaluation point: rank each test label among ALL items the row "
                         "has not seen and report HR@k, NDCG@k (k = 1, 5, 10, 20) and MRR; what counts as seen: 'none' = "
                         "nothing, 'history' = the row's input, 'seen' = every item of the user's training samples and the "
                         "row's input (leave-one-out).  The label itself is never excluded.  'off' = no such evaluation")
    args = ap.parse_args(argv)
    if args.recommend_metrics and not args.recommend_k:
        ap.error("--recommend_metrics measures the lists of --recommend_k: give --recommend_k")
    if (args.recommend_categories or args.recommend_same_category) and not args.recommend_k:
        ap.error("--recommend_categories / --recommend_same_category narrow the lists of --recommend_k: give --recommend_k")
    if args.similar_same_category and not args.similar_k:
        ap.error("--similar_same_category narrows the lists of --similar_k: give --similar_k")
    if args.recommend_explain and not args.recommend_k:
        ap.error("--recommend_explain explains the lists of --recommend_k: give --recommend_k")
    if args.recommend_explain and not 1 <= args.recommend_explain <= 16:
        ap.error("--recommend_explain wants R in 1..16")
    if args.recommend_explain and (args.sharded or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        ap.error("--recommend_explain: Model.explain is single GPU; the sharded form is not built")
    if (args.shelves or args.shelf_items or args.shelf_min_items != 1 or args.shelf_skip_last) and not (args.shelves and args.shelf_items):
        ap.error("--shelves S and --shelf_items M go together; --shelf_min_items / --shelf_skip_last serve them")
    if args.shelves and not args.category_index:
        ap.error("--shelves scans the per-category index: give --category_index 1")
    if args.shelves and not (1 <= args.shelves <= 32 and 1 <= args.shelf_items <= 64 and args.shelves * args.shelf_items <= 256
                             and 1 <= args.shelf_min_items <= args.shelf_items):
        ap.error("--shelves wants S in 1..32, --shelf_items M in 1..64 with S x M <= 256, --shelf_min_items in 1..M")
    if args.shelves and (args.sharded or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        ap.error("--shelves: a category's items are spread over the ranks, so a rank cannot rank categories alone: it is "
                 "not built for the sharded driver")
    if args.category_index and not (args.recommend_categories or args.recommend_same_category or args.similar_same_category
                                    or args.shelves):
        ap.error("--category_index serves --recommend_same_category / --similar_same_category (and --recommend_categories "
                 "with them) and --shelves: give one of them")
    if args.cluster_index and not args.recommend_k:
        ap.error("--cluster_index serves the lists of --recommend_k: give --recommend_k")
    if args.cluster_index and (args.category_index or args.recommend_same_category):
        ap.error("--cluster_index goes without --category_index / --recommend_same_category: a row's lists are chosen by the index")
    if args.cluster_index < 0 or (args.cluster_index and not 1 <= args.cluster_probes <= 64):
        ap.error("--cluster_index wants NLISTS >= 1 and --cluster_probes in 1..64")
    if (args.shortlist_index or args.shortlist) and not args.recommend_k:
        ap.error("--shortlist_index / --shortlist serve the lists of --recommend_k: give --recommend_k")
    if args.shortlist and not args.shortlist_index:
        ap.error("--shortlist is the shortlist index's length: give --shortlist_index 1")
    if args.shortlist_index and (args.cluster_index or args.category_index or args.recommend_same_category or args.recommend_categories):
        ap.error("--shortlist_index serves the whole catalogue: it goes without a scope, a category or another index")
    if (args.recommend_boost or args.recommend_novelty) and not args.recommend_k:
        ap.error("--recommend_boost / --recommend_novelty adjust the lists of --recommend_k: give --recommend_k")
    if (args.recommend_boost or args.recommend_novelty) and args.shortlist_index:
        ap.error("--shortlist_index certifies the model's score, not a boosted one: it goes without --recommend_boost / --recommend_novelty")
    if args.shortlist and not 16 <= args.shortlist <= 256:
        ap.error("--shortlist wants N in 16..256")
    if args.shortlist_index and (args.sharded or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        ap.error("--shortlist_index certifies a row against one table: it is not built for the sharded driver")
    if args.shortlist_index:      # (the first stage's list -- K, or the second stage's pool -- must be shorter than the shortlist)
        first = args.recommend_k if not recommend_settings(args) else (args.recommend_pool or min(256, max(4 * args.recommend_k, 32)))
        short = args.shortlist or min(256, max(4 * first, 64))
        if not first < short:
            ap.error("--shortlist_index: the first stage's list of %d entries (--recommend_k, or the pool of the second stage) "
                     "needs a shortlist longer than that, and the shortlist is %d (--shortlist, at most 256)" % (first, short))
    if args.recommend_pages < 1 or args.audience_pages < 1:
        ap.error("--recommend_pages / --audience_pages: want P >= 1")
    if args.recommend_pages > 1 and not args.recommend_k:
        ap.error("--recommend_pages pages the lists of --recommend_k: give --recommend_k")
    if args.recommend_pages > 1 and recommend_settings(args):
        ap.error("--recommend_pages: the greedy second stage is not a prefix order: it goes without --recommend_diversity / "
                 "--recommend_per_category / --recommend_pool")
    if args.recommend_pages > 1 and args.shortlist_index:
        ap.error("--shortlist_index certifies the head of the list: it goes without --recommend_pages")
    if args.recommend_pages > 1 and (args.recommend_metrics or args.recommend_explain):
        ap.error("--recommend_metrics / --recommend_explain measure and explain lists of --recommend_k entries: they go without "
                 "--recommend_pages")
    if args.audience_pages > 1 and not args.audience_k:
        ap.error("--audience_pages pages the audiences of --audience_k: give --audience_k")
    if args.audience_k < 0 or args.audience_k > 256:
        ap.error("--audience_k: want K in 1..256 (0 = off)")
    if args.audience_k and not args.audience_items.strip():
        ap.error("--audience_k lists the audiences of --audience_items: give --audience_items")
    if (args.audience_items.strip() or args.audience_exclude != "none") and not args.audience_k:
        ap.error("--audience_items / --audience_exclude serve --audience_k: give --audience_k")
    try:
        args.audience_items = [int(c) for c in args.audience_items.split(",") if c.strip()]
    except ValueError:
        ap.error("--audience_items: want item ids separated by commas, e.g. 3,7,12")
    if any(c < 0 for c in args.audience_items):
        ap.error("--audience_items: item ids are non-negative")
    try:
        args.recommend_categories = [int(c) for c in args.recommend_categories.split(",") if c.strip()]
    except ValueError:
        ap.error("--recommend_categories: want category ids separated by commas, e.g. 3,7,12")
    if any(c < 0 for c in args.recommend_categories):
        ap.error("--recommend_categories: category ids are non-negative")
    return args


def sampled_line(n, res):
    """The driver's line of sampled metrics (metrics_from_histogram's dict)."""
    return "Sampled N=%d: " % n + " ".join("%s = %.4f" % (k, v) for k, v in res.items())


def full_ranking_line(mode, res):
    """The driver's line of full-ranking metrics (full_ranking_metrics' dict)."""
    return "Full ranking (exclude=%s): " % mode + " ".join("%s = %.4f" % (k, v) for k, v in res.items())


def list_metrics_line(res):
    """The driver's line of list metrics (ListMetricCounters.result's dict)."""
    return "List metrics: " + " ".join(("%s = %d" if isinstance(v, int) else "%s = %.4f") % (k, v) for k, v in res.items())


def exclude_arg(mode, seen):
    """A flag's exclusion mode -> the `exclude` argument of recommend / sampled_ranks / label_ranks."""
    return {"none": None, "history": "history", "seen": seen}[mode]


def seen_items_for(args, train_set, n_users, device):
    """The seen-items holder when one of the exclusion flags asks for it (built once, from the host train set)."""
    if "seen" not in (args.recommend_exclude, args.eval_neg_exclude, args.eval_rank_exclude, args.audience_exclude):
        return None
    return SeenItems.from_train_set(train_set, n_users, device)


def recommend_path(model_dir, k):
    return os.path.join(model_dir, "recommend_top%d.npz" % k)


def write_recommendations(model_dir, k, user, ids, scores, settings=None, *, why_item=None, why_value=None, why_kind=None):
    """settings: the diversity keywords of recommend (recommend_settings), recorded beside the lists when any is set.
    why_*: the [rows, k, R] explanations of --recommend_explain; without them the file and its keys are unchanged."""
    path = recommend_path(model_dir, k)
    extra = {} if not settings else dict(diversity=np.float64(settings["diversity"]),
                                         per_category=np.int64(settings["per_category"]),
                                         pool=np.int64(settings["pool"] or 0))
    if why_item is not None:
        extra.update(why_item=np.asarray(why_item, np.int32), why_value=np.asarray(why_value, np.float32),
                     why_kind=np.asarray(why_kind, np.int32))
    np.savez(path, user=np.asarray(user, np.int64), ids=np.asarray(ids, np.int32), scores=np.asarray(scores, np.float32),
             **extra)
    return path


def list_metrics_path(model_dir, k):
    return os.path.join(model_dir, "recommend_top%d_metrics.json" % k)


def write_list_metrics(model_dir, k, res, settings=None):
    """The result dict of the lists' measurement beside the lists, with the diversity settings they were made with."""
    path = list_metrics_path(model_dir, k)
    s = settings or {}
    out = dict(res, diversity=float(s.get("diversity", 0.0)), per_category=int(s.get("per_category", 0)),
               pool=int(s.get("pool") or 0))
    with open(path, "w") as f:
        json.dump(out, f, indent=2)
    return path


def recommend_settings(args):
    """The diversity keywords of model.recommend from the flags; {} when none is set (the plain top-K lists)."""
    if not (args.recommend_diversity or args.recommend_per_category or args.recommend_pool):
        return {}
    return dict(diversity=args.recommend_diversity, per_category=args.recommend_per_category,
                pool=args.recommend_pool or None)


def recommend_boost_vector(args, train_set, item_count):
    """The boost of --recommend_boost / --recommend_novelty -> float32 [item_count] host array, or None when neither is
    given: the file's values, ALPHA x item_self_information(train_set, item_count) formed in float32, or their float32
    sum.  A file of another shape or dtype kind is a ValueError."""
    boost = None
    if args.recommend_boost:
        boost = np.load(args.recommend_boost)
        if boost.shape != (item_count,) or boost.dtype.kind not in "fiu":
            raise ValueError("--recommend_boost: want [%d] numbers, got shape %s dtype %s" % (item_count, boost.shape, boost.dtype))
        boost = boost.astype(np.float32)
    if args.recommend_novelty:
        novelty = np.float32(args.recommend_novelty) * item_self_information(train_set, item_count)
        boost = novelty if boost is None else boost + novelty
    return boost


def similar_path(model_dir, k):
    return os.path.join(model_dir, "similar-%d.npz" % k)


SIMILAR_ROWS = 16384   # query items per similar_items call of write_similar


def write_similar(model, model_dir, k, metric, item_count, write=True, same_category=False, index=None):
    """The k nearest items of EVERY item (model.similar_items; collective on a sharded model, where only the process
    with write=True keeps the lists) -> the path of the .npz written: item [I], ids [I, k], scores [I, k].
    same_category: similar_items' (an item's list holds its own category only); index: its CategoryIndex, which goes
    with same_category."""
    ids, scores = [], []
    scoped = dict(same_category=True) if same_category else {}
    if same_category and index is not None:
        scoped["index"] = index
    for i0 in range(0, item_count, SIMILAR_ROWS):
        a, b = model.similar_items(np.arange(i0, min(i0 + SIMILAR_ROWS, item_count)), k, metric=metric, **scoped)
        if write:
            ids.append(a.cpu().numpy())
            scores.append(b.cpu().numpy())
    if not write:
        return None
    path = similar_path(model_dir, k)
    np.savez(path, item=np.arange(item_count, dtype=np.int32), ids=np.concatenate(ids), scores=np.concatenate(scores))
    return path


def audience_path(model_dir, k):
    return os.path.join(model_dir, "audience-%d.npz" % k)


def shelves_path(model_dir, S, M):
    return os.path.join(model_dir, "shelves_%dx%d.npz" % (S, M))


def write_shelves(model, rows, model_dir, S, M, index, exclude, min_items=1, skip_last=False):
    """model.shelves over every test row (the single-GPU driver's) -> the path of the .npz written: users [N], cats
    [N, S], ids [N, S, M], scores [N, S, M] in test-set order.  skip_last: a row is not offered the category of the last
    item of its input (last_item_categories)."""
    parts = []
    for batch, real, _ in rows.launches(True):
        db = model.device_batch(batch, is_test=True)
        skip = model.last_item_categories(db) if skip_last else None
        cats, ids, scores = model.shelves(db, S, M, index=index, exclude=exclude, min_items=min_items, skip=skip)
        parts.append([t[:real].cpu().numpy() for t in (db.u, cats, ids, scores)])
    users, cats, ids, scores = (np.concatenate(x) for x in zip(*parts))
    path = shelves_path(model_dir, S, M)
    np.savez(path, users=users.astype(np.int64), cats=cats.astype(np.int32), ids=ids.astype(np.int32), scores=scores.astype(np.float32))
    return path


def write_audience(model, rows, model_dir, k, items, exclude, write=True, pages=1):
    """The k best test rows for each item of `items` (model.user_vectors over this process's test rows, then
    model.audience; both collective on a sharded model, where only the process with write=True keeps the lists) -> the
    path of the .npz written: item [Q], users [Q, k] (the rows' user ids, -1 where a list ran out), rows [Q, k] (row
    numbers in the order of the user vectors: the test set's on one GPU, rank by rank on a sharded model), scores [Q, k].
    pages=P > 1: audiences of P x k rows, P pages of k (model.audience_deep); the file is named by P x k."""
    launches = list(rows.launches(False))
    users = model.user_vectors([batch for batch, _, _ in launches], real=[real for _, real, _ in launches])
    if pages > 1:
        ids, scores = model.audience_deep(items, k * pages, users, page=k, exclude=exclude)
    else:
        ids, scores = model.audience(items, k, users, exclude=exclude)
    who = users.users_of(ids)                                          # (collective: every rank)
    if not write:
        return None
    path = audience_path(model_dir, k * pages)
    np.savez(path, item=np.asarray(items, np.int32), users=who.cpu().numpy().astype(np.int32),
             rows=ids.cpu().numpy().astype(np.int32), scores=scores.cpu().numpy().astype(np.float32))
    return path


def load_dataset(path):
    if path.endswith(".npz"):
        return load_packed(path)
    with open(path, "rb") as f:  # train.py:131-135
        train_set = pickle.load(f)
        test_set = pickle.load(f)
        counts = pickle.load(f)
        icl = pickle.load(f)
    return PackedSet.from_samples(train_set), PackedSet.from_samples(test_set), tuple(counts), np.asarray(icl, np.int32)


def prepare_model_dir(model_dir, from_scratch, rank=0, barrier=None):
    """train.py:124-127: `from_scratch` wipes and recreates model_dir (rank 0 does it; the others wait at
    `barrier`).  Returns the checkpoint to resume from, or None -- train.py:71-76 reloads
    tf.train.get_checkpoint_state(model_dir).model_checkpoint_path, i.e. the LATEST save, when
    from_scratch is false; here that is the TLSAN-<step> with the largest step (single-file `.npz` of
    Model.save, or the `.replicated.npz` prefix of ShardedModel.save)."""
    if from_scratch:
        if rank == 0:
            if os.path.isdir(model_dir):
                shutil.rmtree(model_dir)
            os.makedirs(model_dir, exist_ok=True)
        if barrier is not None:
            barrier()
        return None
    best = None
    for f in glob.glob(os.path.join(model_dir, "TLSAN-*.npz")):
        m = re.match(r"TLSAN-(\d+)(\.replicated)?\.npz$", os.path.basename(f))
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), f[:-len(".replicated.npz")] if m.group(2) else f)
    if rank == 0:
        os.makedirs(model_dir, exist_ok=True)
    if barrier is not None:
        barrier()
    return None if best is None else best[1]


def epoch_rng(seed=1234):
    """The reference's shuffle stream: `random.seed(1234)` at import (train.py:15) and
    `random.shuffle(train_set)` once per epoch (:191) -- nothing else draws from `random` in between
    (model.py and input.py never touch it), so a private `random.Random(1234)` shuffling the sample
    ORDER in place epoch after epoch visits the samples exactly as the reference's list shuffle does."""
    return random.Random(seed)


# Evaluation launches: the reference feeds its test set in batches of test_batch_size (128) and aggregates per batch
# (train.py:86-118).  What a test row contributes -- whether its pair is ranked right, the rank of its label -- does
# not depend on the rows it shares a batch with (padded session slots are masked), so the kernels run on chunks of
# EVAL_CHUNK rows (the all-items ranking reaches 39 % of the fp32 matrix peak at 4096 rows per launch and 6 % at 128)
# and the reference's per-batch aggregation is formed from slices of the per-row results: same numbers, same order.
EVAL_CHUNK = 4096


def _test_batches(test_set, config, batch_size=None):
    bs = batch_size or config["test_batch_size"]
    if isinstance(test_set, PackedSet):
        return DataInputTest(test_set, bs, config["Ls"])
    from .device_input import DeviceDataInputTest
    return DeviceDataInputTest(test_set, bs, config["Ls"])


def _share(batch, rank, world):
    """This rank's rows of a global batch (contiguous, as even as possible) and how many of them are
    real: a rank without rows gets row 0 as a placeholder (0 real rows), so that every rank takes
    part in every collective."""
    n = len(batch[0])
    lo, hi = n * rank // world, n * (rank + 1) // world
    if hi == lo:
        return tuple(np.asarray(a)[:1] for a in batch), 0
    return tuple(np.asarray(a)[lo:hi] for a in batch), hi - lo


def _equal_share(batch, rank, world):
    """Like _share, padded (by repeating the last row) to ceil(n / world) rows: the evaluation's
    all-gather is equal-sized.  -> (rows, real rows)"""
    part, real = _share(batch, rank, world)
    want = -(-len(batch[0]) // world)
    have = len(part[0])
    if have < want:
        part = tuple(np.concatenate([a, np.repeat(a[-1:], want - have, axis=0)], 0) for a in part)
    return part, real


class EvalRows:
    """All an evaluation knows about the process layout: which test rows this process hands to the model together, and
    how the processes' results combine.  rank None (train()): the whole test set in launches of EVAL_CHUNK rows, a
    multiple of test_batch_size.  Otherwise (train_sharded()): this rank's share of every reference test batch; the sums
    go through an all-reduce on `device`, the gathered rows to rank 0."""

    def __init__(self, test_set, config, rank=None, world=1, group=None, device="cpu"):
        self.test_set, self.config, self.total = test_set, config, len(test_set)
        self.rank, self.world, self.group, self.device = rank, world, group, device

    def launches(self, pad):
        """(rows, real, row0) of every launch of this process, in test-set order: the rows for the model, how many of
        them count (those past `real` only pad a share to the size every rank launches -- what an evaluation that
        all-gathers asks for with `pad` -- or stand in for a share without rows) and the test-set index of rows[0]."""
        bs = self.config["test_batch_size"]
        if self.rank is None:
            chunk = max(EVAL_CHUNK, bs) // bs * bs
            for bi, batch in _test_batches(self.test_set, self.config, chunk):
                row0 = (bi - 1) * chunk
                yield batch, min(chunk, self.total - row0), row0
        else:
            for bi, batch in DataInputTest(self.test_set, bs, self.config["Ls"]):
                part, real = (_equal_share if pad else _share)(batch, self.rank, self.world)
                yield part, real, (bi - 1) * bs + len(batch[0]) * self.rank // self.world

    def units(self, real):
        """The lengths of a launch's pieces that the reference aggregates per batch (train.py:86-118): its test batches
        within a whole launch; a share is one piece, the rank's part of one test batch (possibly empty)."""
        if self.rank is not None:
            return [real]
        bs = self.config["test_batch_size"]
        return [min(bs, real - lo) for lo in range(0, real, bs)]

    def sum(self, t):
        """The exact sum of an int64 / float64 tensor over the processes."""
        if self.world > 1:
            from .dist import allreduce_sum
            t = allreduce_sum(t.to(self.device), self.group)
        return t

    def gather(self, tensors, real):
        """The real rows of every process's tensors, in rank order, on rank 0 (None on the others)."""
        if self.world == 1:
            return [t[:real] for t in tensors]
        from .dist import allgather_rows
        n = allgather_rows(torch.tensor([real], device=tensors[0].device), self.group).tolist()
        got, w = [allgather_rows(t, self.group) for t in tensors], len(tensors[0])
        if self.rank == 0:
            return [torch.cat([g[r * w:r * w + n[r]] for r in range(self.world)]) for g in got]


def _per_row(rows, pad, fn):
    """fn(launch rows, row0) -> per-row device tensor, over this process's launches: the real rows' values as ONE host
    array (one copy per pass) and the lengths of its units."""
    parts, units = [], []
    for batch, real, row0 in rows.launches(pad):
        parts.append(fn(batch, row0)[:real])
        units += rows.units(real)
    return torch.cat(parts).cpu().numpy(), units


def eval_auc(model, test_set, config, rows=None):
    """train.py:86-96: batch AUCs weighted by batch length; a unit's AUC is the reference's float32 mean of 0/1
    (model.py:263), formed on the host from the count, and a rank's sum and the ranks' sums are formed in double."""
    rows = rows or EvalRows(test_set, config)
    model.check_static_overflow()      # (static_rows: a step that did not fit its exchange is reported here at the latest)
    ok, units = _per_row(rows, False, lambda batch, _: model.pairs_ranked_right(batch))
    s, lo = 0.0, 0
    for n in units:
        if n:
            s += float(np.float32(ok[lo:lo + n].sum()) / np.float32(n)) * n
        lo += n
    res = float(rows.sum(torch.tensor([s], dtype=torch.float64))[0]) / rows.total
    model.eval_writer.add_summary(("AUC", res), global_step=model.global_step.eval())     # train.py:91-94
    return res


def eval_prec_recall(model, test_set, config, rows=None, summary=True):
    """train.py:98-118: one pass over the reference's batches for precision, one for recall (cumulative counters, as the
    reference); the label ranks both need are computed once, and a batch's hits are summed over the ranks' shares.
    summary: whether the values also go to the evaluation summary."""
    rows = rows or EvalRows(test_set, config)
    ranks, units = _per_row(rows, True, lambda batch, _: model.label_ranks(batch))
    los = np.cumsum([0] + units)
    hits = rows.sum(torch.from_numpy(np.stack([hits_and_rows(ranks[lo:lo + n]) for lo, n in zip(los, units)]))).cpu().numpy()
    for h in hits:
        prec = model._topk.add_prec(h[:-1], int(h[-1]))
    for h in hits:
        recall = model._topk.add_recall(h[:-1], int(h[-1]))
    prec, recall = [float(x) for x in prec], [float(x) for x in recall]
    if summary:
        model.eval_writer.add_summary([("P@%d" % k, v) for k, v in zip(KS, prec)] +                 # train.py:103-106
                                      [("R@%d" % k, v) for k, v in zip(KS, recall)],                  # :114-117
                                      global_step=model.global_step.eval())
    return prec, recall


class ListMeasurement:
    """The measurement of --recommend_metrics: called with every launch's device lists as recommend_test_set makes
    them, it counts their ListMetrics (labels: the test positives; weights: the training set's self-information) and one
    exposure counter; result() sums both over the processes -> ListMetricCounters.result's dict, on every rank."""

    def __init__(self, model, rows, k, train_set):
        self.model, self.rows, self.k, self.items = model, rows, k, rows.config["item_count"]
        self.weight = torch.as_tensor(item_self_information(train_set, self.items)).to(model.device)
        self.exposure = torch.zeros(self.items, dtype=torch.int32, device=model.device)
        self.counters = ListMetricCounters()

    def __call__(self, db, ids, real):
        ids = ids.clone()
        ids[real:] = -1       # (rows past `real` pad a launch: measured with the others -- the call is collective -- as empty lists)
        m = self.model.list_metrics(ids, labels=db.i, item_weight=self.weight, exposure=self.exposure)
        self.counters.add(ListMetrics(*[f[:real] for f in m]), self.k)

    def result(self):
        self.counters.reduce(self.rows.sum)
        return self.counters.result(self.rows.sum(self.exposure.to(torch.int64)), self.items)


class RecallMeasurement:
    """The recall of --cluster_index with --recommend_metrics: beside every launch's approximate lists it makes the exact
    ones (the same call without the index) and counts, per real row, the exact list's valid ids the approximate list holds;
    result() sums over the processes -> (recall@k, rows).  then: the ListMeasurement to call on as well (None: none)."""

    def __init__(self, model, rows, k, exclude, exact_settings, then=None):
        self.model, self.rows, self.k, self.exclude, self.settings, self.then = model, rows, k, exclude, exact_settings, then
        self.sums = torch.zeros(2, dtype=torch.float64, device=model.device)      # summed per-row recall, rows counted

    def __call__(self, db, ids, real):
        exact = self.model.recommend(db, self.k, exclude=self.exclude, **self.settings)[0][:real]
        n = (exact >= 0).sum(1)
        hit = ((ids[:real, :, None] == exact[:, None, :]) & (exact[:, None, :] >= 0)).any(1).sum(1)
        ok = n > 0
        self.sums += torch.stack([(hit[ok] / n[ok]).to(torch.float64).sum(), ok.sum().to(torch.float64)])
        if self.then is not None:
            self.then(db, ids, real)

    def result(self):
        s = self.rows.sum(self.sums).cpu().numpy()
        return (float(s[0] / s[1]) if s[1] else float("nan")), int(s[1])


class CertifiedShare:
    """The certified share of --shortlist_index: after every launch, how many of its REAL rows the index certified (the rows
    past `real` only pad a launch); result() -> (rows, certified).  then: the hook to call on as well (None: none)."""

    def __init__(self, index, then=None):
        self.index, self.then = index, then
        self.sums = torch.zeros(2, dtype=torch.int64, device=index.device)

    def __call__(self, db, ids, real):
        self.sums += torch.stack([torch.ones_like(self.index.certified[:real], dtype=torch.int64).sum(),
                                  self.index.certified[:real].sum()])
        if self.then is not None:
            self.then(db, ids, real)

    def result(self):
        rows, cert = self.sums.tolist()
        return rows, cert


def recommend_test_set(model, rows, k, exclude, on_lists=None, same_category=False, explain=0, pages=1, **settings):
    """model.recommend over every test row (settings: its diversity keywords and within=) -> (user, ids, scores) host
    arrays in test-set order; None but on rank 0.  explain=R > 0: also (why_item, why_value, why_kind), [rows, k, R], the R
    strongest history sources of every listed item (model.explain on each launch's lists).  on_lists(device batch, ids, real): called with every launch's device
    lists [rows, k] before they leave the device (ListMeasurement).  same_category: every launch's rows get
    category=model.last_item_categories(their batch).  pages=P > 1: lists of P x k entries, P pages of k behind one
    forward (model.recommend_deep)."""
    parts = []
    for batch, real, _ in rows.launches(True):
        db = model.device_batch(batch, is_test=True)
        if same_category:
            settings["category"] = model.last_item_categories(db)
        if pages > 1:
            ids, scores = model.recommend_deep(db, k * pages, page=k, exclude=exclude, **settings)
        else:
            ids, scores = model.recommend(db, k, exclude=exclude, **settings)
        if on_lists is not None:
            on_lists(db, ids, real)
        out = (db.u, ids, scores)
        if explain:
            why = model.explain(db, ids, top=explain)
            out += (why.item, why.value, why.kind)
        parts.append(rows.gather(out, real))
    if parts[0] is not None:
        return tuple(torch.cat(x).cpu().numpy() for x in zip(*parts))


def _histogram(rows, size, fn):
    """[size] exact counts of fn(launch rows, row0) -> per-row integer device tensor over every process's real rows:
    counted on the device, summed over the launches and the processes, read once."""
    hist = None
    for batch, real, row0 in rows.launches(True):
        h = torch.bincount(fn(batch, row0)[:real].long(), minlength=size)
        hist = h if hist is None else hist + h
    return rows.sum(hist).cpu().numpy()


def eval_sampled(model, rows, n, seed, exclude):
    """HR@k / NDCG@k / MRR / AUC_N of every test label among n sampled negatives (sampled_ranks).  A row's negatives
    depend on its position in the test set (row0 + b), so the result does not depend on the launches."""
    res = metrics_from_histogram(_histogram(rows, n + 1, lambda batch, row0: model.sampled_ranks(
        batch, n, seed=seed, row0=row0, exclude=exclude)), n)
    model.eval_writer.add_summary(list(res.items()), global_step=model.global_step.eval())
    return res


def eval_full_ranking(model, rows, exclude):
    """HR@k / NDCG@k / MRR of every test label among ALL items its row's exclusion list does not hold
    (label_ranks(exclude=); None: among all items)."""
    res = full_ranking_metrics(_histogram(rows, rows.config["item_count"], lambda batch, _: model.label_ranks(
        batch, exclude=exclude)))
    model.eval_writer.add_summary([("Full/" + k, v) for k, v in res.items()], global_step=model.global_step.eval())
    return res


def _run(args, say, model, train_set, rows, seen, triples, issue, topk_report, **extra):
    """The flow of the reference's train.py:185-249, written once for train() and train_sharded(), which pass in what
    differs between them:
      rows                          the EvalRows of the test set: every evaluation runs over it
      seen                          the SeenItems holder of the exclusion flags (None when none asks for it)
      triples()                     one epoch of the (shuffled) train_set as (batch, next, after_next) triples (_lookahead2)
      issue(batch, lr, nxt, nxt2)   issues one step, with the batches to announce ahead (None: none) -> the device scalar
                                    that holds the step's loss
      topk_report                   whether P@k / R@k also go to the evaluation summary and their best values into the
                                    closing lines (train.py:103-117, 241-248: train() does, the sharded driver does not)
      extra                         further entries of the result dict."""
    auc_now = lambda: eval_auc(model, rows.test_set, rows.config, rows)
    prec_recall_now = lambda: eval_prec_recall(model, rows.test_set, rows.config, rows, summary=topk_report)
    sampled_now = lambda: eval_sampled(model, rows, args.eval_negatives, args.eval_neg_seed,
                                       exclude_arg(args.eval_neg_exclude, seen))
    full_now = lambda: eval_full_ranking(model, rows, exclude_arg(args.eval_rank_exclude, seen))
    t0 = time.time()
    init_auc = auc_now()
    say("Init AUC: %.4f" % init_auc)
    if args.eval_negatives:
        say(sampled_line(args.eval_negatives, sampled_now()))
    full_mode = args.eval_rank_exclude if args.eval_rank_exclude != "off" else None
    if full_mode:
        say(full_ranking_line(full_mode, full_now()))
    lr = args.learning_rate
    rng = epoch_rng(args.shuffle_seed)  # train.py:15,191 (sharded: the same shuffle on every rank)
    best_auc, history = 0.0, []
    best_prec, best_recall = [0.0] * 6, [0.0] * 6              # train.py:187-188
    prec, recall = [0.0] * 6, [0.0] * 6
    loss_sum = torch.zeros((), dtype=torch.float32, device=model.device)
    done = False
    for _ in range(args.max_epochs):
        train_set.shuffle(rng)  # train.py:191
        for batch, nxt, nxt2 in triples():
            # the reference reads the loss back every step (model.py:229-234); the sum is all the driver
            # uses, so it is accumulated on the device and read at the evaluation points only
            left = (args.max_steps - model.global_step.eval() - 1) if args.max_steps else 2     # steps after this one
            loss_sum += issue(batch, lr, nxt if left >= 1 else None, nxt2 if left >= 2 else None)
            step = model.global_step.eval()
            if step % args.eval_freq == 0:
                auc = auc_now()
                history.append((step, time.time() - t0, auc))
                say("Epoch %d Global_step %d\tTrain_loss: %.4f\tEval_auc: %.4f" %
                    (model.global_epoch_step.eval(), step, float(loss_sum.item()) / args.eval_freq, auc), flush=True)
                loss_sum.zero_()
                if args.eval_negatives:
                    say(sampled_line(args.eval_negatives, sampled_now()))
                if full_mode:
                    say(full_ranking_line(full_mode, full_now()))
                if args.eval_topk:                             # train.py:209-218: P@k / R@k at every evaluation
                    prec, recall = prec_recall_now()
                    say("Precision:\n" + " ".join("@%d = %.4f" % (k, v) for k, v in zip(KS, prec)))
                    say("Recall:\n" + " ".join("@%d = %.4f" % (k, v) for k, v in zip(KS, recall)))
                    if step > 20000:                        # :222-227
                        best_prec = [max(a_, b_) for a_, b_ in zip(best_prec, prec)]
                        best_recall = [max(a_, b_) for a_, b_ in zip(best_recall, recall)]
                if auc > 0.8 and auc > best_auc:  # train.py:228-230
                    best_auc = auc
                    model.save(None)
                best_auc = max(best_auc, auc)
            if step == 150000:  # train.py:232-233
                lr = 0.1
            if args.max_steps and step >= args.max_steps:
                done = True
                break
        say("Epoch %d DONE\tCost time: %.2f" % (model.global_epoch_step.eval(), time.time() - t0), flush=True)  # :235-237
        model.global_epoch_step_op.eval()
        if done:
            break
    if not args.eval_topk or not history:   # (the reference reports what its evaluations saw; make sure there is one)
        prec, recall = prec_recall_now()
    final_auc = auc_now()
    best_auc = max(best_auc, final_auc)
    final_sampled = sampled_now() if args.eval_negatives else None
    final_full = full_now() if full_mode else None
    model.save(None)                                           # train.py:239
    # --category_index: one index over the whole table for the lists that take one (recommend's, over its scope, below)
    whole = model.category_index() if args.category_index and (
        (args.similar_k and args.similar_same_category) or
        (args.recommend_k and args.recommend_same_category and not args.recommend_categories)) else None
    if args.recommend_k:
        settings = recommend_settings(args)
        # (a DevicePackedSet keeps the host set it was made from: the novelty weights are counted on the host)
        measure = ListMeasurement(model, rows, args.recommend_k, getattr(train_set, "ps", train_set)) \
            if args.recommend_metrics else None
        boost = recommend_boost_vector(args, getattr(train_set, "ps", train_set), rows.config["item_count"])
        # (one holder for every launch; every rank builds the same)
        served = settings if boost is None else dict(settings, boost=model.item_boost(boost))
        scope = dict(within=model.item_scope(categories=args.recommend_categories)) if args.recommend_categories else {}
        if args.category_index and args.recommend_same_category:   # (the scope belongs to the index)
            scope = dict(index=model.category_index(**scope) if scope else whole)
        recall_of = None
        if args.cluster_index:                                     # (the scope belongs to the index)
            cindex = model.cluster_index(args.cluster_index, **scope)
            say("Clustered index: %d lists over %d items, max / mean list %d / %.1f, %d k-means iterations"
                % (cindex.lists, cindex.count, cindex.max_list, cindex.mean_list, len(cindex.objective)))
            if args.recommend_metrics:
                recall_of = RecallMeasurement(model, rows, args.recommend_k, exclude_arg(args.recommend_exclude, seen),
                                              dict(served, **scope), then=measure)
            scope = dict(index=cindex, probes=args.cluster_probes)
        share_of = None
        if args.shortlist_index:
            scope = dict(index=model.shortlist_index(), shortlist=args.shortlist or None)
            share_of = CertifiedShare(scope["index"], then=measure)
        rec = recommend_test_set(model, rows, args.recommend_k, exclude_arg(args.recommend_exclude, seen),
                                 on_lists=share_of or recall_of or measure, same_category=bool(args.recommend_same_category),
                                 explain=args.recommend_explain, pages=args.recommend_pages, **served, **scope)
        list_res = measure.result() if measure is not None else None       # (collective: every rank)
        if recall_of is not None:
            say("Clustered index: recall@%d = %.4f against the exact lists over %d rows (%d probes)"
                % ((args.recommend_k,) + recall_of.result() + (args.cluster_probes,)))
        if share_of is not None:
            n_rows, n_cert = shortlist_share = share_of.result()
            say("Shortlist index: %d of %d rows certified (%.4f); the others served by the full scan" % (n_cert, n_rows, n_cert / max(n_rows, 1)))
        if rec is not None:                                    # (rank 0 holds the rows)
            path = write_recommendations(args.model_dir, args.recommend_k * args.recommend_pages, *rec[:3], settings=settings,
                                         **dict(zip(("why_item", "why_value", "why_kind"), rec[3:])))
            say("Recommendations: %s" % path)
            if list_res is not None:
                say(list_metrics_line(list_res))
                say("List metrics: %s" % write_list_metrics(args.model_dir, args.recommend_k, list_res, settings))
    if args.similar_k:
        path = write_similar(model, args.model_dir, args.similar_k, args.similar_metric, rows.config["item_count"],
                             write=rows.rank in (None, 0), same_category=bool(args.similar_same_category), index=whole)
        if path is not None:
            say("Similar items: %s" % path)
    if args.shelves:
        path = write_shelves(model, rows, args.model_dir, args.shelves, args.shelf_items, whole or model.category_index(),
                             exclude_arg(args.recommend_exclude, seen), args.shelf_min_items, bool(args.shelf_skip_last))
        say("Shelves: %s" % path)
    if args.audience_k:
        if max(args.audience_items) >= rows.config["item_count"]:
            raise ValueError("--audience_items: ids must be in [0, %d)" % rows.config["item_count"])
        path = write_audience(model, rows, args.model_dir, args.audience_k, args.audience_items,
                              seen if args.audience_exclude == "seen" else None, write=rows.rank in (None, 0),
                              pages=args.audience_pages)
        if path is not None:
            say("Audience: %s" % path)
    model.train_writer.flush()
    model.eval_writer.flush()
    say("Best test_auc:", best_auc)
    if topk_report:                                            # train.py:241-248
        say("Best precision:\n" + " ".join("@%d = %.4f" % (k, v) for k, v in zip(KS, best_prec)))
        say("Best recall:\n" + " ".join("@%d = %.4f" % (k, v) for k, v in zip(KS, best_recall)))
    if final_sampled is not None:
        say(sampled_line(args.eval_negatives, final_sampled))
    if final_full is not None:
        say(full_ranking_line(full_mode, final_full))
    say("Finished", flush=True)
    res = dict(init_auc=init_auc, best_auc=best_auc, final_auc=final_auc, steps=model.global_step.eval(),
               seconds=time.time() - t0, history=history, prec=prec, recall=recall,
               best_prec=best_prec, best_recall=best_recall, **extra)
    if final_sampled is not None:
        res["sampled"] = final_sampled
    if final_full is not None:
        res["full_ranking"] = final_full
    if args.recommend_k and list_res is not None:
        res["list_metrics"] = list_res
    if args.recommend_k and args.shortlist_index:
        res["shortlist_certified"] = shortlist_share      # (real test rows, certified ones)
    return res


def train(args, data=None):
    """data (optional): (train PackedSet, test PackedSet, (U, I, C), item_cate_list) already in memory
    (tlsan_amd.build_dataset.build_packed) instead of --dataset."""
    say = (lambda *a, **k: None) if args.quiet else print
    train_set, test_set, (U, I, Cc), icl = load_dataset(args.dataset) if data is None else data
    config = {name: getattr(args, name) for name, _, _ in FLAGS}
    config.update(user_count=U, item_count=I, cate_count=Cc, from_scratch=args.from_scratch, quiet=bool(args.quiet))
    say(json.dumps(config, indent=4), flush=True)
    resume = prepare_model_dir(args.model_dir, args.from_scratch)      # train.py:124-127
    model = Model(config, icl, device=args.device, seed=args.seed, norm_mode=args.norm_mode, l2_mode=args.l2_mode,
                  table_dtype=args.table_dtype, matrix_dtype=args.matrix_dtype)
    if resume is not None:                                             # train.py:71-76 (create_model)
        say("Reloading model parameters..", flush=True)
        model.restore(None, resume)
    else:
        say("Created new model parameters..", flush=True)
    seen = seen_items_for(args, train_set, U, model.device)
    if args.device_input:
        from .device_input import DeviceDataInput, DevicePackedSet
        train_set, test_set = DevicePackedSet(train_set, args.device), DevicePackedSet(test_set, args.device)
        train_batches = lambda: DeviceDataInput(train_set, args.train_batch_size, config["Ls"])
    else:
        train_batches = lambda: DataInput(train_set, args.train_batch_size, config["Ls"])

    def issue(batch, lr, nxt, nxt2):
        model.train_async(batch, lr, next_batch=nxt, after_next=nxt2)
        step = model.global_step.eval()
        if args.display_freq and step % args.display_freq == 0:    # train.py:194-195 (add_summary)
            model.train_writer.add_summary(model.train_summary(), global_step=step)
        return model._out[0]

    return _run(args, say, model, train_set, EvalRows(test_set, config), seen,
                triples=lambda: _lookahead2(model.device_batch(b) for _, b in train_batches()), issue=issue,
                topk_report=True)


def _lookahead2(it):
    """(item, next_or_None, one_after_or_None) triples (ShardedModel.train_async(next_batch=, after_next=))."""
    buf = []
    for x in it:
        buf.append(x)
        if len(buf) == 3:
            yield buf[0], buf[1], buf[2]
            buf.pop(0)
    while buf:
        yield buf[0], (buf[1] if len(buf) > 1 else None), None
        buf.pop(0)


def train_sharded(args):
    """The same flow on N GPUs (`python -m torch.distributed.run --nproc-per-node N -m tlsan_amd.train
    --sharded 1 ...`): tables row-sharded over the ranks (tlsan_amd.dist.ShardedModel), every global
    batch of train_batch_size samples split over the ranks -- one SGD step per global batch, exactly
    the single-GPU trajectory up to fp32 summation order -- evaluation over the split test batches."""
    import torch.distributed as dist
    from .dist import ShardedModel
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        rank_, world_ = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
        local = int(os.environ.get("LOCAL_RANK", "0"))
        args.device = "cuda:%d" % local
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", rank=rank_, world_size=world_, device_id=torch.device(args.device))
    rank, world = dist.get_rank(), dist.get_world_size()
    say = print if (rank == 0 and not args.quiet) else (lambda *a, **k: None)
    train_set, test_set, (U, I, Cc), icl = load_dataset(args.dataset)
    config = {name: getattr(args, name) for name, _, _ in FLAGS}
    config.update(user_count=U, item_count=I, cate_count=Cc, from_scratch=args.from_scratch, quiet=bool(args.quiet))
    # flags this path does not implement are refused, not ignored
    if args.table_dtype != "f32":
        raise NotImplementedError("--table_dtype %s: the sharded step keeps fp32 rows" % args.table_dtype)
    if args.norm_mode != "tf18":
        raise NotImplementedError("--norm_mode %s: the sharded step forms the clip norm as TF 1.8 does (tf18)" % args.norm_mode)
    if args.matrix_dtype != "f32":
        raise NotImplementedError("--matrix_dtype %s: the sharded step computes in fp32" % args.matrix_dtype)
    if args.optimizer in LAZY_ADAGRAD_OPTIMIZERS:
        raise NotImplementedError("--optimizer %s: the sharded step has no Adagrad owner update; train it on one GPU" % args.optimizer)
    lazy_opt = args.optimizer.startswith("lazy_")
    if lazy_opt and args.static_rows:
        raise NotImplementedError("--optimizer %s: --static_rows is the lazy-L2 SGD step's form; the lazy optimizers run "
                                  "the step whose exchange sizes follow the batch" % args.optimizer)
    resume = prepare_model_dir(args.model_dir, args.from_scratch, rank,
                               (lambda: dist.barrier()) if world > 1 else None)     # train.py:124-127
    # (the lazy optimizers are the lazy owner update's form whatever --l2_mode says: train() treats both values alike too)
    l2_mode = "lazy" if lazy_opt else (args.l2_mode if args.optimizer == "sgd" else "dense")
    if args.static_rows and l2_mode != "lazy":
        raise NotImplementedError("--static_rows is the lazy-L2 SGD step's form (--l2_mode lazy --optimizer sgd)")
    model = ShardedModel(config, icl, device=args.device, seed=args.seed, l2_mode=l2_mode,
                         static_rows=(True if args.static_rows == 1 else args.static_rows), wire_dtype=args.wire_dtype)
    if resume is not None:                                                          # train.py:71-76
        say("Reloading model parameters..", flush=True)
        model.restore(None, resume)
    dev = model.device
    seen = seen_items_for(args, train_set, U, dev)

    def triples():
        shares = (_share(b, rank, world) + (len(b[0]),) for _, b in DataInput(train_set, args.train_batch_size, config["Ls"]))
        return _lookahead2((model.device_batch(p_), r_, n_) for p_, r_, n_ in shares)

    def issue(share, lr, nxt, nxt2):
        part, real, n_glob = share
        model.train_async(part, lr, next_batch=None if nxt is None else nxt[0],
                          after_next=nxt2[0] if (nxt2 is not None and args.static_rows) else None,
                          weight=real * world / n_glob, sample0=n_glob * rank // world)
        return model.last_loss[0]

    return _run(args, say, model, train_set, EvalRows(test_set, config, rank, world, model.group, dev), seen, triples, issue,
                topk_report=False, world=world)


def main(argv=None):
    args = parse(argv)
    if args.dataset is None:
        raise SystemExit("--dataset is required")
    sharded = args.sharded or int(os.environ.get("WORLD_SIZE", "1")) > 1
    res = train_sharded(args) if sharded else train(args)
    if not sharded or int(os.environ.get("RANK", "0")) == 0:
        print(json.dumps({k: v for k, v in res.items() if k != "history"}))


if __name__ == "__main__":
    main()
