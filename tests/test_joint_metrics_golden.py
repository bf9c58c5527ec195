"""CPU: the PyTorch composition of semstereo_amd.joint_metrics against tests/golden/joint_metrics.npz -- the record of the reference's own
EPE_metric_mask / D1_metric_mask / Thres_metric_mask with mask_img = mask & class, one class, image and estimate at a time
(tests/golden/make_golden_joint_metrics.py) -- and against the calls that are already pinned to the reference: disparity_metrics'
record and SegmentationMetric's joint matrix.

Bounds, those of tests/test_metrics_golden.py for the same columns: per-image EPE (sum / n) within 5e-7 relative of the float32 AND the
float64 record; D1 and Thres (count / n) within (B + 2) * 2^-24 with B = 1 of the float32 record, and the integer count equal to
round(float32 share * n); NaN and 0 exactly where the reference has them.  Against disparity_metrics(mask_img=mask & class): counts
equal, sums within n * 2^-52 relative (two float64 sums of the same n fp32 values, each within (n - 1) * 2^-53 of exact)."""
import os

import numpy as np
import pytest
import torch

from golden import joint_metrics_cases as jc
from golden import metrics_cases as mc
from test_metrics_golden import rel_close

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "golden", "joint_metrics.npz")
TOL_SHARE = (1 + 2) * 2.0 ** -24


@pytest.fixture(scope="module")
def fx():
    return np.load(NPZ)


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    return semstereo_amd


def np_rec(rec):
    return {k: None if v is None else v.cpu().numpy() for k, v in rec.items()}


def sums_close(a, b, n, what):
    """|a - b| <= n * 2^-52 * |b| elementwise, NaN in the same places."""
    a, b, n = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(n, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, a, b)
    ok = ~np.isnan(b)
    err, bound = np.abs(a - b)[ok], (np.broadcast_to(n, b.shape) * 2.0 ** -52 * np.abs(b))[ok]
    if err.size:
        print(f"{what}: largest |difference| / bound {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
    assert np.all(err <= bound), (what, a, b)


def check_record_against_fixture(name, d, rec, fx):
    """What the CPU and the GPU test ask of a float32 run with thresholds=THRESHOLDS: every class, image and estimate."""
    r = np_rec(rec)
    kept, sel = mc.kept(d), fx[f"{name}/cls_sel"]
    B = sel.shape[0]
    assert np.array_equal(r["cls_sel"], sel), name
    assert np.array_equal(r["image"][:, 0], d["mask"].sum((1, 2)).numpy()) and np.array_equal(r["image"][:, 1], (d["gt"] > 0).sum((1, 2)).numpy())
    assert np.array_equal(r["image"][:, 0], sel.sum(1))
    with np.errstate(all="ignore"):                                            # the skip rule from the record's integers
        assert np.array_equal(~(r["image"][:, 0].astype(np.float64) / r["image"][:, 1].astype(np.float64) < 0.1), kept)
    n = sel.astype(np.float64)[None]                                           # [1, B, 7]
    with np.errstate(all="ignore"):
        for key, _plain, _masked, _thr in jc.METRICS:
            num = r["cls_sums"] if key == "EPE" else r["cls_counts"][..., jc.FLAG[key]].astype(np.float64)
            got = np.where(kept[None, :, None], num / n, 0.0)                  # (the reference returns 0 for an image it skips)
            img32, img64 = fx[f"{name}/{key}/image32"], fx[f"{name}/{key}/image64"]
            if key == "EPE":
                rel_close(got, img32, 5e-7, f"{name}/EPE/image32")
                rel_close(got, img64, 5e-7, f"{name}/EPE/image64")
                continue
            rel_close(got, img32, TOL_SHARE, f"{name}/{key}/image32")
            for e in range(img32.shape[0]):
                for b in range(B):
                    for c in range(jc.NCLS + 1):
                        if kept[b] and sel[b, c] > 0 and not np.isnan(img32[e, b, c]):
                            assert sel[b, c] < 2 ** 22
                            want = int(round(float(img32[e, b, c]) * int(sel[b, c])))
                            assert int(r["cls_counts"][e, b, c, jc.FLAG[key]]) == want, (name, key, e, b, c)
    assert not r["cls_counts"][..., 4].any()                                   # the fourth threshold was not given


def joint_by_loop(d, tau=3.0):
    """(all, out, good[n_est]) int64 [B,7,6] from a plain loop over the pixels, written apart from the library."""
    cls, mask, gt = jc.classes(d).numpy(), d["mask"].numpy(), d["gt"].numpy()
    pred = np.argmax(d["logits"].numpy(), axis=1)                              # the first maximum, a NaN counting as the maximum
    B, H, W = gt.shape
    al, out = np.zeros((B, 7, 6), dtype=np.int64), np.zeros((B, 7, 6), dtype=np.int64)
    good = np.zeros((len(d["ests"]), B, 7, 6), dtype=np.int64)
    errs = [np.abs(gt - e.numpy()) for e in d["ests"]]                         # float32
    for b in range(B):
        for h in range(H):
            for x in range(W):
                g, p = cls[b, h, x], pred[b, h, x]
                al[b, g, p] += 1
                if not mask[b, h, x]:
                    out[b, g, p] += 1
                    continue
                for e, err in enumerate(errs):
                    if err[b, h, x] < np.float32(tau):
                        good[e, b, g, p] += 1
    return al, out, good


def run(sa, d, **kw):
    return sa.joint_metrics.joint_metrics(d["ests"], d["logits"], d["gt"], d["labels"], mask=d["mask"], thresholds=jc.THRESHOLDS, **kw)


def test_the_fixture_holds_every_case_and_stays_small(fx):
    assert os.path.getsize(NPZ) < 2 ** 20
    assert all(v.dtype.kind in "fiu" for v in fx.values())
    for name, c in jc.CASES.items():
        assert fx[f"{name}/cls_sel"].shape == (c["B"], 7) and fx[f"{name}/cls_sel"].dtype == np.int64
        for key in mc.COLUMN:
            for k in ("image32", "image64"):
                assert fx[f"{name}/{key}/{k}"].shape == (c["nest"], c["B"], 7), (name, key, k)
    # the cases are what they are meant to be
    assert all(fx[f"{name}/cls_sel"][:, :6].sum() > 0 for name in jc.CASES if name != "nan_image")
    assert fx["plain_b4/cls_sel"][:, :6].min() >= 178 and fx["plain_b4/cls_sel"][:, :6].max() <= 233
    assert fx["odd_23x41/cls_sel"][:, 6].all() and fx["four_ests_mask_img/cls_sel"][:, 6].all()
    d = jc.inputs("edges")
    err = (d["gt"] - d["ests"][0]).abs()[d["mask"]]
    assert all(bool((err == t).any()) for t in (1.0, 2.0, 3.0))                # E on every threshold and on tau
    gap = fx["class_gap/cls_sel"]
    assert gap[0, 2] == 0 and gap[1, 2] > 0 and np.isnan(fx["class_gap/EPE/image32"][:, 0, 2]).all() \
        and not np.isnan(fx["class_gap/EPE/image32"][:, 1, 2]).any()
    d = jc.inputs("class_gap")
    ratio = mc.skip_ratio(d["mask"], d["gt"])
    assert all(not abs(r - 0.1) <= 1e-3 for r in ratio) and mc.kept(d).all()
    assert d["labels"].shape[2] > d["gt"].shape[2] and d["labels"].dtype == torch.uint8


@pytest.mark.parametrize("name", list(jc.CASES))
def test_record_against_the_reference(sa, fx, name):
    d = jc.inputs(name)
    rec = run(sa, d)
    check_record_against_fixture(name, d, rec, fx)
    if d["range_form"]:                                                        # the range evaluated inside is the mask tensor
        rec2 = sa.joint_metrics.joint_metrics(d["ests"], d["logits"], d["gt"], d["labels"], maxdisp=d["maxdisp"], thresholds=jc.THRESHOLDS)
        assert all(torch.equal(rec[k], rec2[k]) for k in rec)
    rec64 = sa.joint_metrics.joint_metrics([e.double() for e in d["ests"]], d["logits"].double(), d["gt"].double(), d["labels"],
                                           mask=d["mask"], thresholds=jc.THRESHOLDS)
    n = fx[f"{name}/cls_sel"].astype(np.float64)[None]
    with np.errstate(all="ignore"):
        got = np.where(mc.kept(d)[None, :, None], rec64["cls_sums"].numpy() / n, 0.0)
    rel_close(got, fx[f"{name}/EPE/image64"], 1e-12, f"{name}/EPE/image64 from float64 inputs")


@pytest.mark.parametrize("name", list(jc.CASES))
def test_record_against_the_pinned_calls(sa, name):
    d = jc.inputs(name)
    rec = run(sa, d)
    r, cls = np_rec(rec), jc.classes(d)
    for c in range(jc.NCLS + 1):
        _, pin = sa.metrics.disparity_metrics(d["ests"], d["gt"], mask=d["mask"], mask_img=d["mask"] & (cls == c),
                                              thresholds=jc.THRESHOLDS, return_record=True)
        counts, sums = pin["counts"].numpy(), pin["sums"].numpy()
        for e in range(len(d["ests"])):
            assert np.array_equal(counts[e, :, 0], r["cls_sel"][:, c]) and np.array_equal(counts[e, :, 1], r["image"][:, 0]) \
                and np.array_equal(counts[e, :, 2], r["image"][:, 1]), (name, c, e)
            assert np.array_equal(counts[e, :, 3:7], r["cls_counts"][e, :, c, :4]), (name, c, e)
            sums_close(r["cls_sums"][e, :, c], sums[e], r["cls_sel"][:, c], f"{name}/class {c}/est{e} sums")
    honest = sa.SegmentationMetric(5, fold=False)
    honest.addBatch(d["logits"], d["labels"])
    assert np.array_equal(r["joint_all"].sum(0), honest.jointMatrix)
    assert np.array_equal(r["joint_all"].sum(0)[:5, :5].astype(np.float64), honest.confusionMatrix)
    al, out, good = joint_by_loop(d)
    assert np.array_equal(r["joint_all"], al) and np.array_equal(r["joint_out"], out) and np.array_equal(r["joint_good"], good)
    assert (r["joint_all"][None] - r["joint_out"][None] - r["joint_good"] >= 0).all()
    assert np.array_equal((r["joint_all"] - r["joint_out"]).sum(2), r["cls_sel"])


def scores_np(m, pool="pixel"):
    return {k: v.cpu().numpy() for k, v in m.scores(pool).items()}


@pytest.mark.parametrize("name", ["plain_b4", "odd_23x41", "edges", "class_gap"])
def test_scores(sa, name):
    d = jc.inputs(name)
    everything = torch.ones_like(d["mask"])
    seg = sa.SegmentationMetric(5, fold=False)
    seg.addBatch(d["logits"], d["labels"])
    iou = seg.scores()["IoU"].numpy()
    finite = [torch.nan_to_num(e, nan=0.0) for e in d["ests"]]                 # (tau = inf passes every finite E)
    m = sa.JointMetric(5, tau=float("inf"), skip_rule=False)
    m.addBatch(finite, d["logits"], d["gt"], d["labels"], mask=everything)
    s = scores_np(m)
    for e in range(len(finite)):
        rel_close(s["IoU3"][e], iou, 1e-12, f"{name}: tau = inf, every pixel in the mask")
    rel_close(s["IoU"], iou, 1e-12, f"{name}: IoU")
    rel_close(s["mIoU"], float(seg.scores()["mIoU"]), 1e-12, f"{name}: mIoU")
    assert s["mIoU3"].shape == (len(finite),) and s["EPE_c"].shape == (len(finite), 5) and s["n_c"].shape == (5,)
    zero = sa.JointMetric(5, tau=0.0, skip_rule=False)
    zero.addBatch(d["ests"], d["logits"], d["gt"], d["labels"], mask=d["mask"])
    z = scores_np(zero)["IoU3"]
    assert np.all(z[~np.isnan(z)] == 0) and not np.isnan(z).all()
    # the three policies move exactly the pixels outside the mask
    ms = {}
    for policy in ("ignore", "pass", "fail"):
        ms[policy] = sa.JointMetric(5, thresholds=jc.THRESHOLDS, skip_rule=False, invalid=policy)
        ms[policy].addBatch(d["ests"], d["logits"], d["gt"], d["labels"], mask=d["mask"])
    st = {k: v.numpy() for k, v in ms["ignore"].state().items()}
    al, out, good = st["joint_all"][:5, :5].astype(np.float64), st["joint_out"][:5, :5].astype(np.float64), st["joint_good"][:, :5, :5]
    assert out.sum() > 0                                                       # (every case here has pixels outside its mask)

    def iou3(inc, gd):
        with np.errstate(all="ignore"):
            return np.stack([np.diag(g) / (inc.sum(1) + inc.sum(0) - np.diag(inc)) for g in gd])
    rel_close(scores_np(ms["ignore"])["IoU3"], iou3(al - out, good), 1e-12, f"{name}: ignore")
    rel_close(scores_np(ms["pass"])["IoU3"], iou3(al, good + out[None]), 1e-12, f"{name}: pass")
    rel_close(scores_np(ms["fail"])["IoU3"], iou3(al, good), 1e-12, f"{name}: fail")
    with np.errstate(all="ignore"):
        rel_close(scores_np(ms["fail"])["IoU"], np.diag(al) / (al.sum(1) + al.sum(0) - np.diag(al)), 1e-12, f"{name}: IoU over every pixel")
    with pytest.raises(ValueError):
        sa.JointMetric(invalid="drop")
    with pytest.raises(ValueError):
        sa.JointMetric().scores()


@pytest.mark.parametrize("name", list(jc.CASES))
def test_pools_against_the_fixture(sa, fx, name):
    d = jc.inputs(name)
    kept = mc.kept(d)
    m = sa.JointMetric(5, thresholds=jc.THRESHOLDS)
    m.addBatch(d["ests"], d["logits"], d["gt"], d["labels"], mask=d["mask"])
    img, pix = scores_np(m, "image"), scores_np(m, "pixel")
    sel = fx[f"{name}/cls_sel"].astype(np.float64)
    for key in mc.COLUMN:
        out_key = key + "_c" if key in ("EPE", "D1") else f"Thres{key[5:]}_c"
        tol = 5e-7 if key == "EPE" else TOL_SHARE
        for tag in ("image32", "image64") if key == "EPE" else ("image32",):
            per = fx[f"{name}/{key}/{tag}"].astype(np.float64)                 # [n_est, B, 7]
            # the batch value the reference forms from them: the mean over the kept images, NaN included; 0 if none is kept
            want = per[:, kept].sum(1) / kept.sum() if kept.any() else np.zeros((per.shape[0], 7))
            rel_close(img[out_key], want[:, :5], tol, f"{name}/{key}/pool=image from {tag}")
            with np.errstate(all="ignore"):                                    # pooled over pixels: shares weighted by the class's pixels
                w = np.where(kept[None, :, None] & (sel[None] > 0), per * sel[None], 0.0).sum(1) / sel[kept].sum(0)[None]
            rel_close(pix[out_key], w[:, :5], tol, f"{name}/{key}/pool=pixel from {tag}")
    assert np.array_equal(pix["n_c"], sel[kept].sum(0)[:5])


def test_additivity_and_state_round_trip(sa):
    d = jc.inputs("plain_b4")
    whole, halves = sa.JointMetric(5, thresholds=jc.THRESHOLDS), sa.JointMetric(5, thresholds=jc.THRESHOLDS)
    whole.addBatch(d["ests"], d["logits"], d["gt"], d["labels"], mask=d["mask"])
    for sl in (slice(0, 2), slice(2, 4)):
        halves.addBatch([e[sl] for e in d["ests"]], d["logits"][sl], d["gt"][sl], d["labels"][sl], mask=d["mask"][sl])
    a, b = whole.state(), halves.state()
    assert set(a) == set(b)
    for k in a:
        if a[k].dtype == torch.int64:
            assert torch.equal(a[k], b[k]), k
    sums_close(b["cls_sums"].numpy(), a["cls_sums"].numpy(), a["cls_sel"].numpy()[None], "two half-batches: sums")
    rel_close(b["image_means"].numpy(), a["image_means"].numpy(), 1e-12, "two half-batches: per-image means")
    assert a["images"].tolist() == [4, 4]
    other = sa.JointMetric(5, thresholds=jc.THRESHOLDS)
    other.load_state(whole.state())
    for k, v in other.state().items():
        assert v.numpy().tobytes() == a[k].numpy().tobytes() and v.data_ptr() != a[k].data_ptr(), k      # (bytes: NaN equals NaN)
    for k, v in other.scores().items():
        assert v.numpy().tobytes() == whole.scores()[k].numpy().tobytes(), k
    other.addBatch(d["ests"], d["logits"], d["gt"], d["labels"], mask=d["mask"])          # a loaded state goes on adding
    assert torch.equal(other.state()["cls_sel"], 2 * a["cls_sel"])
    other.reset()
    assert all(not bool(v.any()) for v in other.state().values())
    with pytest.raises(ValueError):
        other.addBatch(d["ests"] * 2, d["logits"], d["gt"], d["labels"], mask=d["mask"])  # another number of estimates


def test_skip_rule(sa):
    d = jc.inputs("skips")
    assert np.array_equal(mc.kept(d), [False, True, True, True])
    m, rest = sa.JointMetric(5, thresholds=jc.THRESHOLDS), sa.JointMetric(5, thresholds=jc.THRESHOLDS)
    m.addBatch(d["ests"], d["logits"], d["gt"], d["labels"], mask=d["mask"])
    sl = slice(1, 4)
    rest.addBatch([e[sl] for e in d["ests"]], d["logits"][sl], d["gt"][sl], d["labels"][sl], mask=d["mask"][sl])
    a, b = m.state(), rest.state()
    assert a["images"].tolist() == [4, 3] and b["images"].tolist() == [3, 3]
    for k in a:                                                                # the skipped image contributes nothing
        if a[k].dtype == torch.int64 and k != "images":
            assert torch.equal(a[k], b[k]), k
    sums_close(a["cls_sums"].numpy(), b["cls_sums"].numpy(), b["cls_sel"].numpy()[None], "skips: sums without the skipped image")
    rel_close(a["image_means"].numpy(), b["image_means"].numpy(), 1e-12, "skips: per-image means without the skipped image")
    everyone = sa.JointMetric(5, thresholds=jc.THRESHOLDS, skip_rule=False)
    everyone.addBatch(d["ests"], d["logits"], d["gt"], d["labels"], mask=d["mask"])
    assert everyone.state()["images"].tolist() == [4, 4] and int(everyone.state()["cls_sel"].sum()) == int(a["cls_sel"].sum()) + 5
    d = jc.inputs("all_skipped")
    none = sa.JointMetric(5, thresholds=jc.THRESHOLDS)
    none.addBatch(d["ests"], d["logits"], d["gt"], d["labels"], mask=d["mask"])
    assert none.state()["images"].tolist() == [2, 0] and all(not bool(v.any()) for k, v in none.state().items() if k != "images")
    pix, img = scores_np(none, "pixel"), scores_np(none, "image")
    for k in ("EPE_c", "D1_c", "Thres1_c", "IoU3", "mIoU3", "IoU", "mIoU"):
        assert np.isnan(pix[k]).all(), k                                       # 0 / 0 everywhere
    assert not pix["n_c"].any()
    for k in ("EPE_c", "D1_c", "Thres1_c", "Thres2_c", "Thres3_c"):
        assert not img[k].any(), k                                             # the reference's 0 for a batch without a kept image


def test_eval_metrics_joint_keys_and_values(sa):
    d = jc.inputs("odd_23x41")
    out = sa.eval_metrics_joint(d["ests"], d["logits"], d["gt"], d["labels"], d["maxdisp"])
    assert list(out) == ["mIoU3"] + [f"{k}{i}" for i in range(5) for k in ("EPE_c", "D1_c", "IoU3_")]
    assert all(isinstance(v, list) and len(v) == 2 and all(t.dim() == 0 and t.dtype == torch.float64 for t in v) for v in out.values())
    m = sa.JointMetric(5)
    m.addBatch(d["ests"], d["logits"], d["gt"], d["labels"], maxdisp=d["maxdisp"])
    s = m.scores()
    assert float(out["mIoU3"][1]) == float(s["mIoU3"][1]) and float(out["EPE_c3"][0]) == float(s["EPE_c"][0, 3])
    one = sa.eval_metrics_joint(d["ests"][:1], d["logits"], d["gt"], d["labels"], d["maxdisp"])          # lists of one, as scalar_outputs2
    assert all(len(v) == 1 for v in one.values()) and float(one["IoU3_2"][0]) == float(out["IoU3_2"][0])
    avg = sa.EvalAverager("valid")
    avg.update(one)
    avg.update(one)
    assert avg.mean()["IoU3_2"] == float(one["IoU3_2"][0]) and avg.mean()["mIoU3"] == float(one["mIoU3"][0])
    assert "epoch-exact" in sa.eval_metrics_joint.__doc__ and "JointMetric" in sa.eval_metrics_joint.__doc__


def test_the_script_regenerates_the_committed_file(tmp_path):
    from golden import make_golden_joint_metrics as mg
    if not os.path.isdir(mg.REF):
        pytest.skip("the reference is not on this machine")
    path = str(tmp_path / "joint_metrics.npz")
    mg.generate(path)
    new, old = np.load(path), np.load(NPZ)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k
    assert open(path, "rb").read() == open(NPZ, "rb").read()
