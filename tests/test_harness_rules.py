"""Host logic of the dataset loops (CPU): the per-dataset success rule and the CSV / accuracy bookkeeping of
piccolo_amd.localize.write_results — the reference's localize.py:250-297 (Stanford2D-3D-S) and :513-530 (OmniScenes) —, the one
grouping rule (localize._groups) and the one driver (localize._run_dataset) on a canned dataset."""
import csv

import numpy as np

from piccolo_amd import localize


def _table(errs):
    t = np.zeros((len(errs), 16), np.float32)
    for k, (te, re) in enumerate(errs):
        t[k, 13], t[k, 14], t[k, 15] = te, re, 0.5
        t[k, 3:12] = np.eye(3).reshape(-1)
    return t


def test_success_rules_are_per_dataset():
    # localize.py:250  t < 0.2 m and r < rad2deg(0.2) = 11.459 deg ;  localize.py:513  t < 0.1 m and r < 5 deg
    assert localize.stanford_success(0.15, 3.0) and not localize.omniscenes_success(0.15, 3.0)          # between the two in t
    assert localize.stanford_success(0.05, 8.0) and not localize.omniscenes_success(0.05, 8.0)          # between the two in R
    assert localize.stanford_success(0.05, 3.0) and localize.omniscenes_success(0.05, 3.0)
    assert not localize.stanford_success(0.25, 3.0) and not localize.stanford_success(0.05, 11.5)
    assert not localize.omniscenes_success(0.1, 1.0) and not localize.omniscenes_success(0.01, 5.0)     # strict inequalities


def test_write_results_accuracy_per_dataset(tmp_path, capsys):
    errs = [(0.05, 3.0), (0.15, 3.0), (0.05, 8.0), (0.30, 1.0), (float("nan"), float("nan"))]
    files = ["a/f%d.png" % k for k in range(5)]
    gts = {k: (np.zeros(3, np.float32), np.eye(3, dtype=np.float32), k == 4) for k in range(5)}
    header = ["pano_name", "gt_trans", "gt_rot", "skipped?", "OmniLoc_trans", "OmniLoc_rot", "t_error (m)", "r_error (degrees)", "time (s)"]
    out = {}
    for name, rule in (("stanford", localize.stanford_success), ("omniscenes", localize.omniscenes_success)):
        out[name] = localize.write_results(_table(errs), gts, files, None, str(tmp_path / name), name + ".csv", header,
                                           lambda f: [f], rule)
        printed = capsys.readouterr().out
        assert "Final Accuracy : {}".format(out[name]["accuracy"]) in printed and "skipped 1 rooms" in printed
        with open(tmp_path / name / (name + ".csv")) as f:
            rows = list(csv.reader(f))
        assert rows[0] == header and len(rows) == 6 and rows[5][3] == "1" and len(rows[5]) == 4
        assert abs(float(rows[2][6]) - 0.15) < 1e-6 and float(rows[2][8]) == 0.5
    assert out["stanford"]["accuracy"] == 3 / 4 and out["stanford"]["failed"] == ["a/f3.png"]
    assert out["omniscenes"]["accuracy"] == 1 / 4 and out["omniscenes"]["failed"] == ["a/f1.png", "a/f2.png", "a/f3.png"]
    assert out["stanford"]["skipped"] == out["omniscenes"]["skipped"] == ["a/f4.png"]


# ------------------------------------------------------------------------------------------ the grouping rule and the one driver
def _form(indices, skipped=(), keys=None, size=1):
    return list(localize._groups(indices, lambda k: k in skipped, lambda k: (keys or {}).get(k, "a"), size))


def test_groups_of_size_one_are_singletons_and_empty_input_gives_none():
    assert _form(range(4)) == [[0], [1], [2], [3]]
    assert _form(range(4), skipped={2}) == [[0], [1], [3]]
    assert _form([], size=4) == [] and _form(range(3), skipped={0, 1, 2}, size=4) == []


def test_a_skipped_index_neither_joins_nor_splits_a_group():
    assert _form(range(5), skipped={2}, size=4) == [[0, 1, 3, 4]]
    assert _form(range(5), skipped={0, 4}, size=4) == [[1, 2, 3]]


def test_a_key_change_ends_a_group_and_the_size_caps_it():
    keys = {0: "a", 1: "a", 2: "b", 3: "a", 4: "a"}
    assert _form(range(5), keys=keys, size=4) == [[0, 1], [2], [3, 4]]
    assert _form(range(7), size=3) == [[0, 1, 2], [3, 4, 5], [6]]
    assert _form(range(5), keys=keys, size=2) == [[0, 1], [2], [3, 4]]
    assert _form(range(6), skipped={1}, keys={4: "b"}, size=3) == [[0, 2, 3], [4], [5]]


def test_groups_form_over_one_ranks_indices_only():
    n, keys = 9, {6: "b", 7: "b", 8: "b"}
    assert _form(range(0, n, 2), skipped={2}, keys=keys, size=2) == [[0, 4], [6, 8]]
    assert _form(range(1, n, 2), skipped={2}, keys=keys, size=2) == [[1, 3], [5], [7]]


def test_a_full_group_is_handed_out_before_the_next_index_is_looked_at():
    seen = []
    groups = localize._groups(range(4), lambda k: False, lambda k: seen.append(k) or "a", 2)
    assert next(groups) == [0, 1] and seen == [0, 1]
    assert next(groups) == [2, 3] and seen == [0, 1, 2, 3]


class _FakeJob:
    def __init__(self, k, key):
        self.k, self.group_key = k, key


def test_run_dataset_with_a_canned_dataset(tmp_path, capsys):
    """The driver on the host alone: 7 images, image 2 skipped, image 5 of another key, groups of up to 3."""
    import torch
    n, skip, calls = 7, {2}, {"gt": [], "load": [], "groups": [], "report": []}
    files = ["a/f%d.png" % k for k in range(n)]

    def ground_truth(k):
        calls["gt"].append(k)
        return np.full(3, k, np.float32), np.eye(3, dtype=np.float32), k in skip

    def load(k):
        calls["load"].append(k)
        return _FakeJob(k, "b" if k == 5 else "a")

    def localize_group(jobs):
        calls["groups"].append([j.k for j in jobs])
        return [(torch.full((3, 1), float(j.k)), torch.eye(3), torch.tensor(0.5 + j.k), "extra") for j in jobs]

    def report(k, job, result, row):
        assert job.k == k and result[3] == "extra" and float(row[12]) == 0.5 + k
        calls["report"].append(k)

    table = localize._run_dataset(None, str(tmp_path), files, localize._Dataset(ground_truth, load, localize_group, report), 3, "fake.csv",
                                  ["pano_name", "gt_trans", "gt_rot", "skipped?", "t", "R", "t_err", "r_err", "time (s)"], lambda f: [f],
                                  localize.stanford_success).numpy()
    assert calls["groups"] == [[0, 1, 3], [4], [5], [6]]                   # the skipped image splits nothing; the key and the cap do
    assert calls["load"] == calls["report"] == [0, 1, 3, 4, 5, 6]          # loaded once each, reported once each, in image order
    assert calls["gt"] == list(range(n))                                   # memoised: once per image, though row and CSV read it again
    assert table.shape == (n, 16) and np.isnan(table[2]).all() and not np.isnan(np.delete(table, 2, axis=0)).any()
    for k in (0, 1, 3, 4, 5, 6):                                           # every row at its image's index: t = (k, k, k) = gt_trans
        assert (table[k, 0:3] == k).all() and table[k, 12] == 0.5 + k and table[k, 13] == 0.0
    assert table[0, 15] == table[1, 15] == table[3, 15] and (table[[0, 4, 5, 6], 15] >= 0).all()      # one shared wall time per group
    assert capsys.readouterr().out.count("corrupted file : a/f2.png") == 1
    assert localize.LAST_RUN["total"] == 6 and localize.LAST_RUN["skipped"] == ["a/f2.png"]
    with open(tmp_path / "fake.csv") as f:
        rows = list(csv.reader(f))
    assert len(rows) == n + 1 and [r[3] for r in rows[1:]] == ["0", "0", "1", "0", "0", "0", "0"]
