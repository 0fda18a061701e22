"""Cell-sharded MultiMat objects from feature-major input: MultiMat.from_csmat_inner / from_adaptive_vecs_inner /
from_file against the route a caller had before, the host-transposed triplet handed to MultiMat(...). Everything up to the solvers is
integer work and compared with np.array_equal: the whole matrix, the shard ranges, every shard's arrays, create_info against
host_plan_inner and the uploaded bytes against 8 z + 8 (n + 1) per slab. All shards share device 0."""
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import reshard_ref as ref  # noqa: E402

CLI = os.path.join(ROOT, "scan-rs_amd", "lib", "scan-rs-cmd")
GOLDEN = os.path.join(TESTS, "golden")
MESSAGE = "indices must be in range and strictly ascending within each outer vector"


@pytest.fixture(scope="module")
def sa():
    import scanrs_amd

    if not scanrs_amd.device_available():
        pytest.fail("gpu tests need a gfx950 device")
    return scanrs_amd


@functools.lru_cache(maxsize=None)
def case(name):
    """(n_outer, n_inner, triplet, host-transposed triplet with its stored zeros, the same with them dropped), computed once."""
    n_outer, n_inner, ip, ix, vv = ref.CASES[name]()
    t = ref.transposed_triplet(ip, ix, vv, n_outer, n_inner)
    for a in (ip, ix, vv) + t:
        a.setflags(write=False)
    return n_outer, n_inner, (ip, ix, vv), t, ref.drop_zeros(*t)


def shape_of(sa, storage, n_outer, n_inner):
    """feature-major CSR: features x cells; cell-row CSC: cells x features with the same arrays"""
    return (n_outer, n_inner) if storage == sa.CSR else (n_inner, n_outer)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("n_shards", ref.SHARDS)
@pytest.mark.parametrize("storage_name", ["csr", "csc"])
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_inner_equals_host_transposed(sa, name, storage_name, n_shards):
    storage = sa.CSR if storage_name == "csr" else sa.CSC
    other = sa.CSC if storage == sa.CSR else sa.CSR
    n_outer, n_inner, (ip, ix, vv), (tip, tix, tvv), dropped = case(name)
    rows, cols = shape_of(sa, storage, n_outer, n_inner)
    dev = [0] * n_shards
    mm = sa.MultiMat.from_csmat_inner(rows, cols, storage, ip, ix, vv, n_shards, devices=dev)
    assert mm.storage == other and mm.shape() == [rows, cols] and mm.n_shards == n_shards
    # the whole matrix: the scipy transposition with the stored zeros removed
    got = mm.to_csmat()
    m = sp.csr_matrix((vv.copy(), ix.astype(np.int64), ip.astype(np.int64)), shape=(n_outer, n_inner))
    m.eliminate_zeros()
    t = m.tocsc()
    t.sort_indices()
    assert same(got, (t.indptr.astype(np.uint64), t.indices.astype(np.uint32), t.data.astype(np.uint32)))
    assert same(got, dropped) and mm.nnz() == int(np.count_nonzero(vv))
    # the shard ranges: plan_shards of the transposed indptr, stored zeros counted
    bounds = sa.plan_shards(tip, n_shards)
    assert [(lo, hi) for _, lo, hi in mm.shard_ranges()] == [(int(bounds[i]), int(bounds[i + 1])) for i in range(n_shards)]
    # every shard: the arrays of the shard the host route makes
    host = sa.MultiMat(rows, cols, other, tip, tix, tvv, n_shards, devices=dev)
    assert host.shard_ranges() == mm.shard_ranges()
    for i in range(n_shards):
        assert same(mm.shard_csmat(i), host.shard_csmat(i)), f"shard {i}"
    # what the constructor did, against the host plan; every slab uploaded once
    info = mm.create_info()
    sb, bd, mv = sa.host_plan_inner(ip, ix, n_inner, n_shards)
    assert np.array_equal(info["slab_bounds"], sb) and np.array_equal(bd, bounds) and np.array_equal(info["moved"], mv)
    z = ip[sb[1:].astype(np.int64)] - ip[sb[:-1].astype(np.int64)]
    assert np.array_equal(info["uploaded_bytes"], 8 * z + 8 * (sb[1:] - sb[:-1] + 1))
    assert int(info["uploaded_bytes"].sum()) == 8 * ix.size + 8 * (n_outer + n_shards)


@pytest.fixture(scope="module")
def inner_of(sa):
    """from_csmat_inner of a case over 3 shards (feature-major CSR) as (to_csmat, shard ranges), made once per case"""
    @functools.lru_cache(maxsize=None)
    def make(name):
        n_outer, n_inner, (ip, ix, vv), _, _ = case(name)
        mm = sa.MultiMat.from_csmat_inner(n_outer, n_inner, sa.CSR, ip, ix, vv, 3, devices=[0] * 3)
        return mm.to_csmat(), mm.shard_ranges(), [mm.shard_csmat(i) for i in range(3)]

    return make


@pytest.fixture(scope="module")
def single_of(sa):
    @functools.lru_cache(maxsize=None)
    def make(name):
        n_outer, n_inner, (ip, ix, vv), _, _ = case(name)
        return sa.AdaptiveMat.from_csmat(n_outer, n_inner, sa.CSR, ip, ix, vv)

    return make


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5, 6, 7, None])
@pytest.mark.parametrize("name", ["seeded", "long_vector"])
def test_adaptive_vecs_inner(sa, inner_of, single_of, name, kind):
    n_outer, n_inner, _, _, _ = case(name)
    vecs = single_of(name).to_adaptive_vecs(kind)
    assert len(vecs) == n_outer
    mm = sa.MultiMat.from_adaptive_vecs_inner(n_outer, n_inner, sa.CSR, vecs, 3, devices=[0] * 3)
    whole, ranges, shards = inner_of(name)
    assert mm.storage == sa.CSC and same(mm.to_csmat(), whole) and mm.shard_ranges() == ranges
    for i in range(3):
        assert same(mm.shard_csmat(i), shards[i])
    info = mm.create_info()
    units = np.concatenate([[0], np.cumsum([v["n_units"] for v in vecs])]).astype(np.uint64)
    assert np.array_equal(info["slab_bounds"], sa.plan_shards(units, 3))  # the slabs are cut by the entries the vectors store
    assert int(info["moved"].sum()) == whole[1].size and np.all(info["uploaded_bytes"][np.diff(info["slab_bounds"]) > 0] > 0)


def write_mtx(path, m):
    coo = m.tocoo()
    with gzip.open(path, "wt") as f:
        f.write("%%MatrixMarket matrix coordinate integer general\n")
        f.write(f"{m.shape[0]} {m.shape[1]} {coo.nnz}\n")
        for i in np.random.default_rng(0).permutation(coo.nnz):  # unsorted triplets
            f.write(f"{coo.row[i] + 1} {coo.col[i] + 1} {coo.data[i]}\n")


def seeded_scipy():
    n_outer, n_inner, (ip, ix, vv), _, _ = case("seeded")
    return sp.csr_matrix((vv.copy(), ix.astype(np.int64), ip.astype(np.int64)), shape=(n_outer, n_inner))


@pytest.mark.parametrize("which", ["h5", "mtx"])
def test_from_file(sa, tmp_path, which):
    from scanrs_amd import hdf5_io, mtx

    if which == "h5":
        path = os.path.join(GOLDEN, "tiny_10x.h5")
        fm, _ = hdf5_io.read_adaptive_csr_matrix(path)
    else:
        path = os.path.join(tmp_path, "matrix.mtx.gz")
        write_mtx(path, seeded_scipy())
        fm = mtx.load_mtx(path)
    assert fm.storage == sa.CSR and fm.nnz > 0
    a = sa.MultiMat.from_file(path, 3, devices=[0, 0, 0])
    b = sa.MultiMat.from_csmat_inner(fm.rows, fm.cols, fm.storage, fm.indptr, fm.indices, fm.values, 3, devices=[0, 0, 0])
    c = fm.to_devices(3, devices=[0, 0, 0])
    for x in (a, c):
        assert x.storage == sa.CSC and x.shape() == [fm.rows, fm.cols] and x.shard_ranges() == b.shard_ranges()
        assert same(x.to_csmat(), b.to_csmat())
        assert all(np.array_equal(x.create_info()[k], b.create_info()[k]) for k in ("slab_bounds", "moved", "uploaded_bytes"))


def test_downstream(sa):
    """normalize + BkSvd, group_sums and kNN on (a) over 3 shards: the shards are those of the host route, so the same code runs on the
    same arrays and U, sigma, V must be EQUAL; against one handle made from the CSR triplet sigma agrees to the suite's bound for
    shards against one handle (1e-8 relative), and the integer results are equal."""
    from scanrs_amd import sseq
    import select_sharded_case as sel

    n_outer, n_inner, (ip, ix, vv), (tip, tix, tvv), _ = case("seeded")
    k = 7
    mm = sa.MultiMat.from_csmat_inner(n_outer, n_inner, sa.CSR, ip, ix, vv, 3, devices=[0, 0, 0])
    host = sa.MultiMat(n_outer, n_inner, sa.CSC, tip, tix, tvv, 3, devices=[0, 0, 0])
    labels = sel.seeded_labels()
    one = sa.AdaptiveMat.from_csmat(n_outer, n_inner, sa.CSR, ip, ix, vv)
    sums1, cnt1 = sseq.group_sums(one, labels, sel.N_GROUPS)
    sums, cnt = sseq.group_sums(mm, labels, sel.N_GROUPS)
    assert np.array_equal(sums, sums1) and np.array_equal(cnt, cnt1)
    u, s, v = mm.normalize(sa.Normalization.CellRanger).run_pca_bk(k)
    uh, sh, vh = host.normalize(sa.Normalization.CellRanger).run_pca_bk(k)
    print("sigma (inner-sharded) ", s, "\nsigma (host-transposed)", sh)
    assert np.array_equal(s, sh) and np.array_equal(u, uh) and np.array_equal(v, vh)
    u1, s1, v1 = sa.BkSvd().run_pca(sa.normalize(one, sa.Normalization.CellRanger), k)
    rel = float(np.max(np.abs(s - s1) / s1))
    print("sigma against one handle: max relative difference", rel)
    assert rel < 1e-8
    assert np.array_equal(mm.knn(5, points=v1), sa.knn(v1, 5))


def in_use(sa):
    sa.release_cached_memory()
    return sa.device_memory_in_use()


def test_refusals(sa):
    n_outer, n_inner, (ip, ix, vv), (tip, tix, tvv), _ = case("seeded")
    sb = sa.plan_shards(ip, 3)
    last = n_outer - 1
    assert int(sb[2]) <= last and int(ip[last + 1]) - int(ip[last]) >= 2  # the last vector lies in the last slab
    before = in_use(sa)

    def refused(indices, n_shards, text, code=6, n_dev=None):
        with pytest.raises(sa.ScanrsError) as e:
            sa.MultiMat.from_csmat_inner(n_outer, n_inner, sa.CSR, ip, indices, vv, n_shards, devices=[0] * (n_shards if n_dev is None else n_dev))
        assert e.value.code == code and text in str(e.value), str(e.value)
        assert in_use(sa) == before

    unsorted = ix.copy()
    a = int(ip[last])
    unsorted[a], unsorted[a + 1] = unsorted[a + 1], unsorted[a]
    refused(unsorted, 3, MESSAGE)
    beyond = ix.copy()
    beyond[int(ip[last + 1]) - 1] = n_inner  # still ascending, one past the last position
    refused(beyond, 3, MESSAGE)
    refused(beyond, 1, MESSAGE)
    refused(ix, 0, "1 <= n_shards <= 16")
    refused(ix, 17, "1 <= n_shards <= 16")
    plain = sa.MultiMat(n_outer, n_inner, sa.CSC, tip, tix, tvv, 2, devices=[0, 0])
    with pytest.raises(sa.ScanrsError) as e:
        plain.create_info()
    assert e.value.code == 6 and "inner-sharding constructor" in str(e.value)
    plain.close()
    assert in_use(sa) == before


def read_csv(path):
    with gzip.open(path, "rt") as f:
        return np.array([[float(x) for x in line.strip().split(",")] for line in f if line.strip()])


def test_cli_gpus(sa, tmp_path):
    mtx = os.path.join(tmp_path, "m.mtx.gz")
    write_mtx(mtx, seeded_scipy())
    out3, out1 = os.path.join(tmp_path, "out3"), os.path.join(tmp_path, "out1")
    r = subprocess.run([CLI, mtx, "-o", out3, "--gpus", "3", "--devices", "0,0,0", "-n", "cellranger", "-d", "7"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    u, d, v = (read_csv(os.path.join(out3, f"svd_{x}.csv.gz")) for x in "udv")
    u2, s2, v2 = sa.MultiMat.from_file(mtx, 3, devices=[0, 0, 0]).normalize(sa.Normalization.CellRanger).run_pca_bk(7)
    assert np.array_equal(d[:, 0], s2) and np.array_equal(u, u2) and np.array_equal(v, v2)  # CSV round-trips f64 exactly
    r = subprocess.run([CLI, mtx, "-o", out1, "-n", "cellranger", "-d", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    d1 = read_csv(os.path.join(out1, "svd_d.csv.gz"))
    rel = float(np.max(np.abs(d[:, 0] - d1[:, 0]) / d1[:, 0]))
    print("sigma, --gpus 3 against the run without --gpus: max relative difference", rel)
    assert rel < 1e-8
    for bad in (["--gpus", "0"], ["--gpus", "2", "--devices", "0,x"], ["--gpus", "2", "--devices", "0,0,0"], ["--gpus", "2", "--devices", "0,,0"]):
        r = subprocess.run([CLI, mtx, "-o", out1, "-d", "7"] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and ("--gpus" in r.stderr or "--devices" in r.stderr), (bad, r.stderr)
