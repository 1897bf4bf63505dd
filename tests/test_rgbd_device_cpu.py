"""cvo_rgbd_frame_rows_host, the CPU twin of the rows and the exclusion rule a device RGB-D frame's cloud is made of, against
the numpy statement (np_rgbd_device): np_rgbd.points / np_rgbd.recipe rows padded to 5 features and 19 classes, the first
maximum over STRIDED class scores.  Every comparison is of bit patterns.  No GPU."""
import numpy as np
import pytest

import np_rgbd_device as nd
import rgbd_cases as rc
import rgbd_device_cases as dc
from unified_cvo_amd import CvoError, RGBDFrame, _capi, rgbd_frame_rows_host, rgbd_points_host

DSO_EDGES, FULL = dc.DSO_EDGES, dc.FULL

FRAMES = ("tiny", "small", "mono", "semantic")
METHODS = {"dso": DSO_EDGES, "full": FULL}
LEAF = 0.1


@pytest.mark.parametrize("depth", rc.DEPTHS)
@pytest.mark.parametrize("name", FRAMES)
def test_rows_equal_the_statement(name, depth):
    f = rc.frame(name, depth)
    for mname, method in METHODS.items():
        want = dc.statement_points(f, method)
        got = rgbd_frame_rows_host(f, want["pixel"], method)
        assert got["feat"].shape[1] == nd.FEATURES
        dc.assert_rows_equal(got, want, (name, depth, mname))
        assert (got["label"] is None) == (f.semantic is None)
        if f.semantic is not None:
            assert got["label"].shape[1] == nd.CLASSES and not got["excluded"].any()   # (the statement kept these pixels)
    r = dc.statement_recipe(f, LEAF)
    got = rgbd_frame_rows_host(f, r["pixel"], recipe=True, is_edge=r["is_edge"])
    assert r["is_edge"].any() and not r["is_edge"].all()
    dc.assert_rows_equal(got, r, (name, depth, "recipe"), labels=False)


def test_exclusion_of_every_pixel_equals_the_statement():
    f = rc.frame("semantic")
    want = nd.excluded(f.semantic)
    assert want.any() and not want.all()
    got = rgbd_frame_rows_host(f, np.arange(f.rows * f.cols), FULL)
    assert np.array_equal(got["excluded"], want)
    assert np.array_equal(rc.bits(got["label"]), rc.bits(nd.labels_of(f.semantic, np.arange(f.rows * f.cols))))


def test_three_presentations_of_one_plane_give_identical_bytes():
    f = rc.frame("semantic")
    want = dc.statement_points(f, DSO_EDGES)
    pixel, every = want["pixel"], np.arange(f.rows * f.cols)
    seen = []
    for name, (base, view, layout) in dc.presentations(f.semantic).items():
        assert np.array_equal(nd.hwc(view, layout), f.semantic), name           # the same scores, presented differently
        assert np.array_equal(nd.excluded(view, layout), nd.excluded(f.semantic)), name
        got = rgbd_frame_rows_host(f, pixel, DSO_EDGES, semantic=view, layout=layout)
        dc.assert_rows_equal(got, dc.statement_points(f, DSO_EDGES, view, layout), name)
        excl = rgbd_frame_rows_host(f, every, FULL, semantic=view, layout=layout)["excluded"]
        assert np.array_equal(excl, nd.excluded(view, layout)), name
        seen.append(b"".join(got[k].tobytes() for k in ("xyz", "feat", "label", "geotype")) + excl.tobytes())
    assert seen[0] == seen[1] == seen[2]


@pytest.mark.parametrize("name", sorted(dc.RULE_CASES))
def test_exclusion_rule_edges(name):
    f = dc.rule_frame(name)
    want_excl = nd.excluded(f.semantic)
    if dc.RULE_EXCLUDES[name]:
        assert want_excl.any() and not want_excl.all(), name        # the statement excludes some pixels and keeps some
    else:
        assert f.num_classes <= 10 and not want_excl.any(), name    # no class 10: it cannot win
    got = rgbd_frame_rows_host(f, dc.all_pixels(), FULL)
    assert np.array_equal(got["excluded"], want_excl), name
    want = dc.statement_points(f, FULL)
    assert set(want["pixel"].tolist()) == set(np.flatnonzero(~want_excl).tolist())   # every pixel has a depth: FULL keeps what the rule keeps
    dc.assert_rows_equal(rgbd_frame_rows_host(f, want["pixel"], FULL), want, name)


def test_shared_maxima_and_equal_scores_by_hand():
    f = dc.rule_frame("shared_10_12")
    s = f.semantic
    both = (s[..., 10] == s.max(axis=2)) & (s[..., 12] == s.max(axis=2))
    assert both.any() and np.array_equal(nd.excluded(s).reshape(dc.H, dc.W)[both], np.ones(both.sum(), bool))     # 10 comes first: excluded
    f = dc.rule_frame("shared_3_10")
    s = f.semantic
    both = (s[..., 3] == s.max(axis=2)) & (s[..., 10] == s.max(axis=2))
    assert both.any() and not nd.excluded(s).reshape(dc.H, dc.W)[both].any()                                       # 3 comes first: kept
    f = dc.rule_frame("all_equal")
    s = f.semantic
    flat = (s == s[..., :1]).all(axis=2)
    assert flat.any() and not nd.excluded(s).reshape(dc.H, dc.W)[flat].any()                                       # class 0: kept
    for name in ("shared_10_12", "shared_3_10", "all_equal"):
        f = dc.rule_frame(name)
        assert np.array_equal(rgbd_frame_rows_host(f, dc.all_pixels(), FULL)["excluded"], nd.excluded(f.semantic)), name


def test_nan_scores_follow_the_existing_host_entry_point():
    """np.argmax treats a NaN as the maximum and upstream's behaviour on NaN scores is not pinned, so this one case is compared
    with the existing cvo_rgbd_points_host only: `row[c] > row[best]` never lets a NaN win and never replaces a NaN at best = 0."""
    f = dc.nan_frame()
    assert np.isnan(f.semantic).any()
    pc = rgbd_points_host(f, FULL)
    kept = np.zeros(dc.H * dc.W, bool)
    kept[pc.pixel] = True
    got = rgbd_frame_rows_host(f, dc.all_pixels(), FULL)
    assert np.array_equal(got["excluded"], ~kept)
    assert kept.any() and not kept.all()
    v = lambda y, x: y * dc.W + x
    assert kept[v(0, 0)] and kept[v(0, 1)] and kept[v(2, 2)] and not kept[v(0, 2)] and not kept[v(1, 1)]
    rows = rgbd_frame_rows_host(f, pc.pixel, FULL)
    assert np.array_equal(rc.bits(rows["label"]), rc.bits(nd.pad(pc.labels(), nd.CLASSES)))
    assert np.array_equal(rc.bits(rows["xyz"]), rc.bits(pc.positions())) and np.array_equal(rc.bits(rows["feat"]), rc.bits(nd.pad(pc.features(), nd.FEATURES)))


def test_last_pixel_and_border_pixels():
    f = dc.rule_frame("classes_19")
    want = dc.statement_points(f, FULL)
    last = dc.H * dc.W - 1
    assert last in want["pixel"].tolist()          # its gradient index p + 1 = h w is read as pixel (h w) / 2: in bounds
    got = rgbd_frame_rows_host(f, want["pixel"], FULL)
    dc.assert_rows_equal(got, want, "classes_19")
    edge = dc.border(want["pixel"])
    half = np.float32(0.5)
    assert edge.any() and not edge.all()
    # feature 3 is gradient_[p], the gradient of pixel p / 2; feature 4 of pixel (p + 1) / 2: both 0 -> 0.5 where THAT pixel is on the border
    for col, src in ((3, want["pixel"] // 2), (4, (want["pixel"] + 1) // 2)):
        on_border = dc.border(src)
        assert on_border.any() and np.all(got["feat"][on_border, col] == half)
    big = rc.frame("tiny")
    every = np.arange(big.rows * big.cols)
    got = rgbd_frame_rows_host(big, every, FULL)   # every pixel, with or without a depth: the rows of the border read no neighbour
    ref = dc.statement_points(RGBDFrame(big.image, np.ones_like(big.depth), big.fx, big.fy, big.cx, big.cy, big.scaling_factor), FULL)
    order = np.argsort(ref["pixel"], kind="stable")
    assert np.array_equal(ref["pixel"][order], every)
    assert np.array_equal(rc.bits(got["feat"]), rc.bits(ref["feat"][order]))


def test_own_gray_plane():
    f = rc.own_gray(rc.frame("tiny"))
    for method in METHODS.values():
        want = dc.statement_points(f, method)
        dc.assert_rows_equal(rgbd_frame_rows_host(f, want["pixel"], method), want, "own gray")
    plain = rc.frame("tiny")
    want = dc.statement_points(plain, FULL)
    assert not np.array_equal(rgbd_frame_rows_host(f, want["pixel"], FULL)["feat"], want["feat"])   # the plane is what the gradient is taken of


def test_refusals():
    f = rc.frame("tiny")
    with pytest.raises(CvoError) as e:
        rgbd_frame_rows_host(f, [f.rows * f.cols], FULL)          # a pixel outside the image
    assert e.value.code == _capi.CVO_E_INVALID
    with pytest.raises(CvoError):
        rgbd_frame_rows_host(f, [-1], FULL)
    with pytest.raises(CvoError) as e:
        rgbd_frame_rows_host(f, [0], 0)                           # CV_FAST
    assert e.value.code == _capi.CVO_E_UNSUPPORTED
    with pytest.raises(ValueError, match="is_edge"):
        rgbd_frame_rows_host(f, [0, 1], recipe=True)
    sem = np.zeros((f.rows, f.cols, 20), np.float32)
    with pytest.raises(CvoError) as e:
        rgbd_frame_rows_host(f, [0], FULL, semantic=sem)          # 20 classes
    assert e.value.code == _capi.CVO_E_UNSUPPORTED
    assert rgbd_frame_rows_host(f, [], FULL)["xyz"].shape == (0, 3)
