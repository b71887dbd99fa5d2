"""CPU checks of the inputs test_scene_edges_gpu.py runs on the device (tests/scene_edge_cases.py): each edge a GPU case aims at
is asserted here from the numpy model alone (oracle/dataset_oracle.py), so that no GPU case passes because its edge never
occurred.  A seed that fails a condition is replaced, the condition stays."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_edge_cases as C  # noqa: E402


# ======================================================================================================================
# A. voxel down-sampling
# ======================================================================================================================
@pytest.mark.parametrize("origin", C.FACE_ORIGINS)
@pytest.mark.parametrize("vs", (0.05, 0.1))
def test_a1_face_lattice_separates_the_division_from_its_imitations(vs, origin):
    pts, j, _, _ = C.face_cloud(vs, origin)
    assert len(pts) == 4000 and (pts[j[:, 0] == 0] == origin).all() and (pts.min(axis=0) == origin).all()
    got = C.face_counts(pts, j, vs)
    print("vs %g origin %g: %s" % (vs, origin, got))
    assert got["total"] == 3 * C.FACE_POINTS
    assert got["integer"] >= 1000      # a quotient that is an exact integer: the coordinate lies on the face itself
    assert got["below"] >= 1000        # a floor below j: the rounding of p put it into the voxel before
    assert got["reciprocal"] >= 1000   # (p - min_bound) * (1 / vs) lands in another voxel than the true division
    assert got["float32"] >= 1000      # and so does a float32 quotient


@pytest.mark.parametrize("origin", C.FACE_ORIGINS)
def test_a1_quarter_voxels_are_the_exact_control(origin):
    pts, j, _, _ = C.face_cloud(0.25, origin)
    got = C.face_counts(pts, j, 0.25)
    assert got["integer"] == got["total"] and got["below"] == 0 and got["reciprocal"] == 0


@pytest.mark.parametrize("vs", C.FACE_VS)
def test_a1_voxels_have_several_members(vs):
    pts, j, _, labels = C.face_cloud(vs, 0.0)
    vox = C.voxel_index(pts, vs)
    _, counts = np.unique(vox, axis=0, return_counts=True)
    assert counts.max() >= 3 and (counts >= 2).sum() >= 500 and labels.min() >= 1 and labels.max() <= 8


def _one_voxel_means(pts, cols):
    fwd = C.voxel_down_sample(pts, cols, None, 1.0)
    rev = C.voxel_down_sample(pts[::-1], cols[::-1], None, 1.0)
    return fwd, rev


def test_a2_the_sum_of_one_voxel_depends_on_the_order():
    pts, cols, _ = C.sum_order_cloud(C.SUM_MEMBERS)
    assert len(pts) == 3001 and np.log10(pts.max() / pts[pts > 0].min()) > 9  # ten decades
    fwd, rev = _one_voxel_means(pts, cols)
    assert len(fwd[0]) == 1 and len(rev[0]) == 1          # one voxel
    assert (fwd[0] != rev[0]).any() and (fwd[1] != rev[1]).any()  # the reversed input has another mean: points and colours


def test_a2_the_wide_voxel_stands_beside_single_member_voxels():
    pts, cols, _ = C.sum_order_cloud(C.SUM_MEMBERS_WIDE, C.SUM_SINGLES)
    vox = C.voxel_index(pts, 1.0)
    _, counts = np.unique(vox, axis=0, return_counts=True)
    assert sorted(counts.tolist()) == [1] * C.SUM_SINGLES + [C.SUM_MEMBERS_WIDE]
    big = (vox == 0).all(axis=1)
    assert big.sum() == C.SUM_MEMBERS_WIDE and not big[:100].all() and not big[-100:].all()  # interleaved with the singles
    fwd, rev = _one_voxel_means(pts[big], cols[big])
    assert (fwd[0] != rev[0]).any() and (fwd[1] != rev[1]).any()


def test_a3_counts_stand_next_to_the_block_and_grid_boundaries():
    assert set(C.COUNTS_SMALL) == {1, 2, 255, 256, 257, 1023, 1024, 1025}
    assert C.COUNTS_LARGE == (256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1)  # 256 threads x 1024 workgroups: the grid-stride cap
    assert max(C.COUNTS_LARGE) <= 300000
    for n in C.COUNTS_SMALL:
        pts, cols, labels = C.count_cloud(n)
        assert pts.shape == (n, 3) and cols.shape == (n, 3) and labels.shape == (n,)
        nvox = len(np.unique(C.voxel_index(pts, C.COUNT_VS), axis=0))
        if n == 2:
            assert (pts[0] == pts[1]).all() and nvox == 1
        elif n > 2:
            assert 2.0 <= n / nvox <= 8.0  # about four members per voxel
    pts = C.count_cloud(C.COUNTS_LARGE[1])[0]
    assert pts.min() >= -3 and pts.max() <= 3


def test_a4_the_order_cloud_holds_every_kind_of_neighbour():
    pts, _, _, planned = C.order_cloud()
    vox = C.voxel_index(pts, C.ORDER_VS)
    assert np.array_equal(vox, np.array(C.ORDER_INDICES)[planned])  # every point in the voxel it was planned for
    uniq = np.unique(vox, axis=0)  # sorted lexicographically by (ix, iy, iz)
    assert len(uniq) == len(C.ORDER_INDICES)
    step = np.diff(uniq, axis=0)
    assert ((step[:, 0] == 0) & (step[:, 1] == 0) & (step[:, 2] != 0)).any()  # neighbours in the output differing only in iz
    assert ((step[:, 0] == 0) & (step[:, 1] != 0)).any() and (step[:, 0] != 0).any()
    as_set = {tuple(v) for v in uniq.tolist()}
    assert {(5, 7, 9), (5, 7, 10), (5, 8, 9), (6, 7, 9)} <= as_set  # only iz, only iy, only ix apart
    assert uniq[:, 0].max() == 2 ** 21 - 1 and uniq[:, 1].max() == 2 ** 21 - 1 and uniq[:, 2].max() == 2 ** 21 - 1
    key = (uniq[:, 0] << 42) | (uniq[:, 1] << 21) | uniq[:, 2]
    assert (key >> 62).max() == 1 and (np.diff(key) > 0).all()  # bit 62 is set; key order == (ix, iy, iz) order
    # the input is not sorted already, and the model's output is
    in_key = (vox[:, 0] << 42) | (vox[:, 1] << 21) | vox[:, 2]
    assert (np.diff(in_key) < 0).any()
    sp = C.voxel_down_sample(pts, None, None, C.ORDER_VS)[0]
    out = np.floor((sp - (pts.min(axis=0) - C.ORDER_VS * 0.5)) / C.ORDER_VS).astype(np.int64)
    assert np.array_equal(out, uniq)
    assert np.bincount(planned).min() >= 2  # several members everywhere


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_a5_extents_at_the_21_bit_limit(axis):
    fits = C.voxel_index(C.limit_cloud(axis, C.EXTENT_FITS)[0], C.LIMIT_VS)
    over = C.voxel_index(C.limit_cloud(axis, C.EXTENT_OVER)[0], C.LIMIT_VS)
    assert fits.max() == fits[1, axis] == 2097151 and fits.sum() == 2097151
    assert over.max() == over[1, axis] == 2097152 and over.sum() == 2097152


def test_a6_label_votes():
    pts, cols, labels = C.label_cloud()
    vox = C.voxel_index(pts, C.LABEL_VS)
    assert np.array_equal(vox[:, 0], [0, 0, 0, 0, 1, 1, 1, 2, 3, 3, 3]) and not vox[:, 1:].any()
    assert labels[vox[:, 0] == 0].tolist() == [5, 3, 5, 3]  # a tie, the larger label first
    assert C.voxel_model(pts, cols, labels, C.LABEL_VS)[2].tolist() == [3, 63, 8, 2]
    assert C.voxel_model(pts, cols, None, C.LABEL_VS)[2] is None
    assert not C.voxel_model(pts, None, labels, C.LABEL_VS)[1].any()


def test_a7_signed_zeros_and_subnormals_are_there():
    pts, _, _ = C.signed_zero_cloud()
    neg = np.signbit(pts) & (pts == 0)
    assert neg[:, 0].any() and (~neg[:, 0] & (pts[:, 0] == 0)).any()  # x: a minimum of -0.0 beside +0.0
    assert (pts.min(axis=0) == 0).all() and neg[:, 1].any() and neg[:, 2].any() and not np.signbit(pts[0]).any()
    sp = C.voxel_model(pts, None, None, 0.05)[0]
    assert not np.signbit(sp[0]).any() and (sp[0] == 0).all()  # the model: 0.0 + -0.0 = +0.0
    pts, cols, _ = C.subnormal_cloud()
    tiny = np.finfo(np.float64).tiny
    assert ((pts > 0) & (pts < tiny)).sum() >= 15 and ((cols > 0) & (cols < tiny)).sum() >= 15
    sp, sc, _ = C.voxel_model(pts, cols, None, 0.05)
    assert ((sp[0] > 0) & (sp[0] < tiny)).all() and ((sc[0] > 0) & (sc[0] < 1)).all()  # a subnormal mean


def test_a9_the_plain_cloud_is_finite_and_the_rows_are_the_ends_and_the_middle():
    pts, _, labels = C.plain_cloud()
    assert np.isfinite(pts).all() and len(pts) == 1000 and labels.min() >= 1
    assert C.NONFINITE_ROWS == (0, 500, 999)
    assert np.isnan(C.NONFINITE_VALUES[0]) and C.NONFINITE_VALUES[1:] == (np.inf, -np.inf)


# ======================================================================================================================
# B. the single-scene sampler
# ======================================================================================================================
def test_b1_lattice_centres_have_all_four_kinds_of_face_point():
    o = C.oracle_of(C.lattice_scene())
    p = o.points
    assert (p * 2 == np.round(p * 2)).all()
    zsize = p[:, 2].max() - p[:, 2].min()
    saw = set()
    for xyz in C.LATTICE_CENTERS:
        ci = C.find_point(o, xyz)
        cx, cy, cz = p[ci]
        idx = C.column(o, ci)
        inside = np.zeros(len(p), dtype=bool)
        inside[idx] = True
        in_yz = (np.abs(p[:, 1] - cy) <= C.HALF) & (np.abs(p[:, 2] - cz) <= zsize)
        right, left = (p[:, 0] == cx + C.HALF) & in_yz, (p[:, 0] == cx - C.HALF) & in_yz
        assert right.sum() > 1 and not inside[right].any()   # x == box_max: outside
        assert left.sum() > 1 and inside[left].all()         # x == box_min: inside
        for side in (-1, 1):
            face = (p[:, 1] == cy + side * C.HALF) & (np.abs(p[:, 0] - cx) < C.HALF)
            assert face.sum() > 1 and inside[face].all()     # y == box_min / box_max: inside
            zface = (p[:, 2] == cz + side * zsize) & (np.abs(p[:, 0] - cx) < C.HALF) & (np.abs(p[:, 1] - cy) <= C.HALF)
            if zface.any():
                assert inside[zface].all()                   # z == cz -+ scene_z_size: inside
                saw.add(side)
        # the x faces fall inside runs of equal x values: the search has to stop at the run's first row
        i_min, i_max = C.slab(o, ci)
        assert p[i_min, 0] == cx - C.HALF == p[i_min + 1, 0] and p[i_min - 1, 0] < cx - C.HALF
        assert p[i_max, 0] == cx + C.HALF == p[i_max + 1, 0] and p[i_max - 1, 0] < cx + C.HALF
        assert len(idx) > C.LATTICE_NPTS
    assert saw == {-1, 1}  # both z faces occurred among the centres


def test_b2_first_and_last_point_reach_the_ends_of_the_scene():
    o = C.oracle_of(C.ends_scene())
    n = len(o.points)
    assert n == 700 < 1024
    assert C.slab(o, 0)[0] == 0 and C.slab(o, 0)[1] < n
    assert C.slab(o, n - 1)[1] == n and C.slab(o, n - 1)[0] > 0
    assert len(C.column(o, 0)) > C.ENDS_NPTS and len(C.column(o, n - 1)) > C.ENDS_NPTS


def test_b3_slabs_of_1023_1024_1025_and_3000_rows():
    o = C.oracle_of(C.chunk_scene())
    for k, size in enumerate(C.CHUNK_SLABS):
        ci = C.block_center(o, k)
        i_min, i_max = C.slab(o, ci)
        assert i_max - i_min == size
        idx = C.column(o, ci)
        assert len(idx) == size - size // 2 and (np.diff(idx) > 0).all()  # half inside in y, in scene order
        assert idx[0] >= i_min and idx[-1] < i_max and not np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx)))
        assert len(idx) > C.CHUNK_NPTS


@pytest.mark.parametrize("npts", C.COUNT_NPTS)
def test_b4_column_counts_around_npts(npts):
    o = C.oracle_of(C.count_scene(npts))
    centers, masks, cap = C.count_plan(o, npts)
    want = [1, 2, npts - 1, npts, npts + 1, npts + 1, npts + 1, 3 * npts + 7]
    got = [C.sample_model(o, ci, masks[s], npts) for s, ci in enumerate(centers)]
    assert [g["cnt"] for g in got] == want and cap == 3 * npts + 7
    assert np.array_equal(got[3]["sel"], got[3]["idx"])            # cnt == npts: the repeat branch is the identity
    assert np.array_equal(got[0]["sel"], np.repeat(got[0]["idx"], npts))
    assert np.array_equal(got[2]["sel"], np.concatenate((got[2]["idx"], got[2]["idx"][:1])))  # npts - 1: the first row again
    for s, drop in zip((4, 5, 6), (0, (npts + 1) // 2, npts)):    # npts + 1: exactly one row dropped
        assert masks[s].sum() == npts and np.array_equal(got[s]["sel"], np.delete(got[s]["idx"], drop))
    assert masks[7].sum() == npts and masks[7, :want[7]].sum() == npts and all(len(g["sel"]) == npts for g in got)


def test_b8_centring_in_float32_would_differ_far_from_the_origin():
    o = C.oracle_of(C.far_scene())
    masks = C.random_masks(o, C.FAR_CENTERS, C.FAR_NPTS, len(o.points), 181)
    for s, ci in enumerate(C.FAR_CENTERS):
        m = C.sample_model(o, ci, masks[s], C.FAR_NPTS)
        assert m["cnt"] > C.FAR_NPTS
        raw32 = m["raw"].astype(np.float32)
        box_min = raw32.min(axis=0)
        shift32 = np.array([box_min[0] + np.float32(C.HALF), box_min[1] + np.float32(C.HALF), box_min[2]], dtype=np.float32)
        early = raw32 - shift32
        assert early.dtype == np.float32 and (early != m["centered"]).mean() > 0.5  # the cast first: most values differ


def test_b9_a_scene_without_labels_and_colours_is_all_zero_in_the_model():
    pts, _, _ = C.ends_scene()
    o = C.oracle_of((pts, None, None))
    m = C.sample_model(o, 10, C.random_masks(o, [10], C.ENDS_NPTS, len(pts), 5)[0], C.ENDS_NPTS)
    assert not m["labels"].any() and not m["colors"].any() and m["raw"].any()
