"""CPU tests of the clustered item index: the numpy reference itself (tests/cluster_ref.py) -- its objective never rises,
full probing unions to all items, ties and NaN in the probe order -- the fixtures of the GPU tests against the 1 % cap on
excused results (tests/cluster_cases.py; the reference alone), and the host-side plumbing of tlsan_amd/cluster.py:
ClusteredIndex.from_assignment on device "cpu" against tests/lists_ref.index_of, the max_list= splitting, every ValueError
that needs no GPU, the exports."""
import os
import re

import numpy as np
import pytest

from tests import cluster_cases as cases, cluster_ref as cref, lists_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_objective_never_rises_and_planted_clusters_are_found():
    vec, _, _, lab = cases.planted_table()
    train, init = cases.fit_draws(cases.PLANTED_I, cases.PLANTED_LISTS, cases.FIT_SEED)
    assert np.array_equal(train, np.arange(600)) and len(set(init.tolist())) == 12
    cent, a, objective, margin = cref.fit(vec, init, 10)
    assert 2 <= len(objective) < 10 and all(z <= y for y, z in zip(objective, objective[1:]))
    assert margin > 10.0                                                # the fit fixture: far beyond the fp32 bound
    assert len(np.unique(a)) == 12 and a.shape == (600,)
    # Lloyd from random rows splits some planted clusters and merges others: every list is dominated by one label
    assert np.mean([np.bincount(lab[a == j]).max() / (a == j).sum() for j in range(12)]) > 0.8
    x2 = cases.gauss(600, 64, 5)
    _, _, obj2, _ = cref.fit(x2, np.arange(12), 10)
    assert all(z <= y for y, z in zip(obj2, obj2[1:]))


def test_reference_means_and_assign_basics():
    x = cases.gauss(50, 64, 1)
    cent = x[[3, 10, 10, 20]].copy()                                    # centroids 1 and 2 are equal
    a, dist, sure, _ = cref.assign(x, cent)
    assert a[3] == 0 and a[10] == 1 and a[20] == 3 and dist[3] == 0.0 and dist[10] == 0.0    # a tie goes to the lower id
    assert not (a == 2).any() and not sure[10]
    xn = x.copy()
    xn[4, 7] = np.nan
    assert cref.assign(xn, cent)[0][4] == 0                             # a row whose best value is NaN
    order = np.array([5, 6, 7, 1])
    got = cref.means(x, order, [0, 3, 3, 4, 4], cent)
    assert np.array_equal(got[0], x[[5, 6, 7]].astype(np.float64).mean(0).astype(np.float32))
    assert np.array_equal(got[1], cent[1]) and np.array_equal(got[2], x[1]) and np.array_equal(got[3], cent[3])


def test_reference_probe_order_ties_nan_empty_and_fill():
    s = np.array([1.0, 3.0, np.nan, 3.0, -0.0, 0.0, -np.inf])
    assert cref.probe_order(s).tolist() == [1, 3, 0, 4, 5, 6, 2]        # equal -> the lower list; +0 == -0; NaN last
    assert cref.probe_order(s, np.array([1, 0, 1, 1, 1, 0, 1], bool)).tolist() == [3, 0, 4, 6, 2]
    q, cent = cases.gauss(5, 64, 2), cases.gauss(3, 64, 3)
    off = np.array([0, 2, 2, 5])
    rows = cref.probe(q, cent, 4, list_off=off)
    assert (rows[:, 2:] == -1).all() and (np.sort(rows[:, :2], 1) == [0, 2]).all()          # C < P, an empty list
    assert cref.recall([[1, 2, 3, -1]], [[3, 1, 9, 8]]) == 0.5 and np.isnan(cref.recall([[1]], [[-1]]))


def test_full_probing_unions_to_all_items():
    from tlsan_amd.cluster import ClusteredIndex
    rng = np.random.RandomState(3)
    assign = rng.randint(0, 9, 500)
    assign[assign == 4] = 5                                             # an empty list
    cent = cases.gauss(9, 64, 4)
    for max_list in (None, 25):
        ci = ClusteredIndex.from_assignment(assign, cent, max_list=max_list)
        off, items = ci.partition.list_off.numpy(), ci.partition.list_items.numpy()
        rows = cref.probe(cases.gauss(7, 64, 5), ci.centroids.numpy(), min(64, ci.lists), list_off=off)
        ok = lists_ref.union_mask(7, 500, rows, off, items)
        assert ok.all() and (rows >= 0).sum(1).tolist() == [ci.nonempty] * 7


def test_the_gpu_fixtures_keep_the_cap_on_the_reference():
    for d in cases.DS:
        for nc in cases.ASSIGN_C:
            x, cent = cases.assign_case(d, nc)
            assert (~cref.assign(x, cent)[2]).mean() <= 0.01, (d, nc)
        for name, q, cent, P, kw in cases.probe_cases(d):
            assert (~cref.probe_sure(q, cent, P, **kw)).mean() <= 0.01, name
    names = [c[0] for d in cases.DS for c in cases.probe_cases(d)]
    assert len(set(names)) == len(names) and sum(n.startswith("d64") for n in names) == 4 * 4 * 4


def test_from_assignment_on_the_cpu_is_the_reference_index():
    import torch
    from tlsan_amd.cluster import ClusteredIndex
    from tlsan_amd.model import CategoryIndex, ItemScope
    rng = np.random.RandomState(7)
    assign = rng.randint(0, 6, 300)
    assign[assign == 2] = 0
    cent = cases.gauss(6, 128, 8)
    cent[5] = 0.0
    item_b = rng.randn(300).astype(np.float32)
    for within in (None, np.arange(0, 300, 7)):
        scope = None if within is None else ItemScope(300, "cpu", items=within)
        ci = ClusteredIndex.from_assignment(torch.as_tensor(assign), torch.as_tensor(cent), "cpu", item_b=item_b, within=scope)
        off, items = lists_ref.index_of(assign, 6, within=within)
        assert isinstance(ci.partition, CategoryIndex) and ci.partition.cate_count == 6 == ci.lists == ci.nlists
        assert np.array_equal(ci.partition.list_off.numpy(), off) and np.array_equal(ci.partition.list_items.numpy(), items)
        assert ci.max_list == int(np.diff(off).max()) and ci.count == len(items) and ci.nonempty == int((np.diff(off) > 0).sum())
        assert np.array_equal(ci.centroids.numpy(), cent) and ci.centroids.dtype == torch.float32
        want_b = [item_b[items[off[c]:off[c + 1]]].astype(np.float64).mean() if off[c + 1] > off[c] else 0.0 for c in range(6)]
        assert np.allclose(ci.list_bias.numpy(), want_b, rtol=1e-7, atol=0) and ci.list_bias.numpy()[2] == 0.0
        inv = ci.centroid_inv.numpy()
        assert inv[5] == 0.0 and np.allclose(inv[:5], 1.0 / np.sqrt((cent[:5].astype(np.float64) ** 2).sum(1)), rtol=1e-7)
        loc = ci.partition.local(4, 1, 75)                               # the sharded-ready layout comes with the partition
        assert int(loc[0][-1]) == int(((items % 4 == 1) & (items // 4 < 75)).sum())
    with pytest.raises(RuntimeError):
        ci.probe(torch.zeros(2, 128), 2)                                 # no CPU fallback


def test_max_list_splits_oversized_lists():
    from tlsan_amd.cluster import ClusteredIndex
    rng = np.random.RandomState(9)
    assign = rng.choice(5, 400, p=[0.6, 0.2, 0.15, 0.05, 0.0])           # a skewed partition, list 4 empty
    cent = cases.gauss(5, 64, 10)
    item_b = rng.randn(400)
    whole = ClusteredIndex.from_assignment(assign, cent, item_b=item_b)
    ci = ClusteredIndex.from_assignment(assign, cent, item_b=item_b, max_list=30)
    off, items, parent = ci.partition.list_off.numpy(), ci.partition.list_items.numpy(), ci.parent.numpy()
    sizes = np.diff(off)
    assert ci.max_list == sizes.max() <= 30 and ci.lists == len(parent) == len(sizes) > 5 and ci.nlists == 5
    assert sizes.sum() == 400 and (np.diff(parent) >= 0).all() and sorted(set(parent.tolist())) == [0, 1, 2, 3, 4]
    for c in range(5):
        mine = np.concatenate([items[off[l]:off[l + 1]] for l in np.nonzero(parent == c)[0]])
        assert np.array_equal(mine, np.nonzero(assign == c)[0])          # consecutive chunks, ids ascending
        full = sizes[parent == c]
        assert (full[:-1] == 30).all() and (len(full) == max(1, -(-int((assign == c).sum()) // 30)))
    assert np.array_equal(ci.centroids.numpy(), cent[parent])            # the parents' centroids, bias and norm
    assert np.array_equal(ci.list_bias.numpy(), whole.list_bias.numpy()[parent])
    assert np.array_equal(ci.centroid_inv.numpy(), whole.centroid_inv.numpy()[parent])
    same = ClusteredIndex.from_assignment(assign, cent, max_list=1000)
    assert same.lists == 5 and np.array_equal(same.partition.list_off.numpy(), whole.partition.list_off.numpy())


def test_value_errors_that_need_no_gpu():
    from tlsan_amd.cluster import ClusteredIndex, clustered_probes
    from tlsan_amd.dist import refuse_clustered
    from tlsan_amd.model import CategoryIndex, ItemScope
    cent = cases.gauss(4, 64, 1)
    ci = ClusteredIndex.from_assignment(np.arange(40) % 4, cent)
    cat = CategoryIndex(np.arange(40) % 4, 4, "cpu")
    assert clustered_probes(None, None, 40) is None and clustered_probes(cat, None, 40, category=[1]) is None
    assert clustered_probes(ci, 3, 40, category=None, within=None, same_category=False) == 3
    assert clustered_probes(ci, 64, 40) == 64
    for args, kw in (((None, 3, 40), {}), ((cat, 3, 40), {}),                              # probes= without a clustered index
                     ((ci, None, 40), {}), ((ci, 0, 40), {}), ((ci, 65, 40), {}), ((ci, 2.5, 40), {}), ((ci, True, 40), {}),
                     ((ci, 3, 41), {}),                                                   # an index over another item count
                     ((ci, 3, 40), dict(category=[0])), ((ci, 3, 40), dict(within=ItemScope(40, "cpu", items=[1]))),
                     ((ci, 3, 40), dict(same_category=True))):
        with pytest.raises(ValueError):
            clustered_probes(*args, **kw)
    for bad in (dict(assign=np.arange(40) % 5), dict(assign=-np.ones(40, np.int64)), dict(assign=np.zeros((4, 10), np.int64)),
                dict(assign=np.zeros(40)), dict(centroids=cases.gauss(4, 96, 1)), dict(centroids=np.zeros(64, np.float32)),
                dict(max_list=0), dict(within=[1, 2]), dict(within=ItemScope(41, "cpu", items=[1])), dict(item_b=np.zeros(39)),
                dict(assign=np.arange(40000) % 4, max_list=1)):                            # more than 16384 lists
        kw = dict(assign=np.arange(40) % 4, centroids=cent)
        kw.update(bad)
        with pytest.raises(ValueError):
            ClusteredIndex.from_assignment(kw.pop("assign"), kw.pop("centroids"), **kw)
    with pytest.raises(TypeError):
        ClusteredIndex()
    refuse_clustered(None)
    refuse_clustered(cat)
    for args in ((ci,), (ci, 3), (None, 3), (cat, 3)):
        with pytest.raises(ValueError, match="ClusteredIndex"):
            refuse_clustered(*args)


def test_the_library_exports_the_cluster_calls():
    from tlsan_amd import _lib as L, build
    names = ("tlsan_cluster_workspace_bytes", "tlsan_cluster_assign", "tlsan_cluster_means", "tlsan_cluster_probe")
    with open(os.path.join(ROOT, "include", "tlsan.h")) as f:
        header = f.read()
    lib = L.load()
    for name in names:
        assert name in L.EXPORTS and hasattr(lib, name) and re.search(r"\b%s\(" % name, header), name
    assert "tlsan_cluster.hip" in build.SOURCES and L.ABI_VERSION == 15 and lib.tlsan_abi_version() == 15
    assert lib.tlsan_cluster_workspace_bytes(0, 16384, 0) >= 4 * 16384
    assert lib.tlsan_cluster_workspace_bytes(4096, 1024, 64) >= 4 * 4096 * 64
    assert lib.tlsan_cluster_workspace_bytes(4, 16385, 2) == 0 and b"tlsan_cluster_workspace_bytes" in lib.tlsan_last_error()
    # the three calls refuse bad arguments before any launch, with their own names (no GPU is touched)
    assert lib.tlsan_cluster_assign(None, 1, 64, None, 1, None, None, None, 0, None) == -1
    assert lib.tlsan_last_error().startswith(b"tlsan_cluster_assign")
    assert lib.tlsan_cluster_means(None, 1, None, None, 1, 64, None, None) == -1
    assert lib.tlsan_last_error().startswith(b"tlsan_cluster_means")
    assert lib.tlsan_cluster_probe(None, 1, 64, None, None, None, None, 1, 1, None, None, 0, None) == -1
    assert lib.tlsan_last_error().startswith(b"tlsan_cluster_probe")
