"""TEST INFRASTRUCTURE ONLY: the plain numpy restatement of matrix construction on the device, and the cases the CPU and GPU tests
share (tests/test_construct_cpu.py, tests/test_gpu_construct.py, tests/test_gpu_adaptive_decode.py).

What the library does in scan-rs_amd/csrc/copy_build.hip and decode.hip, said once more without any of its arithmetic:

  transpose     the transposed copy: a stable sort on the inner index, so outer ids ascend inside every inner vector
  validate      (violations, stored zeros, largest count) by a walk over the outer vectors: the definition, not the streaming formula
  compact       stored zeros dropped, the vectors closed up (AbsIter skips stored zeros)
  sort_within   (index, count) pairs sorted by index inside every outer vector (the repair of unsorted 10x files)
  items         the pieces of at most ITEM_NNZ nonzeros every outer vector is worked in
  select_outer / select_inner   the two selections, for the copies a select adopts
  product / product_t           A X and A^T Y in u32 (sums wrap modulo 2^32)

Decode expectations do not come from here: they are `iter()` of oracle/adaptive_vec.py, the reference's AbsIter.

Everything is integer work on (indptr u64, indices u32, values u32) of an n_outer x n_inner copy, the outer vectors stored one after
the other. Cases are seeded builders; each is built once per process (functools.lru_cache) and its arrays are read-only."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import adaptive_grid as ag  # noqa: E402
import adaptive_vec as av  # noqa: E402

ITEM_NNZ = 8192           # nonzeros per work item (common.hpp)
U32_MAX = 2**32 - 1
PACKED, PAIR = 1, 2       # counter "transpose_route" / host_transpose_plan
MI355X_CUS = 256          # the CPU tests size the grid-stride case with it; the GPU tests read the device's own count
STREAM_CHUNK = 4          # validate_stream_kernel reads the nonzeros four at a time


def stream_span(n_cu):
    """nonzeros one trip of validate_stream_kernel's grid-stride loop covers: n_cu * 16 workgroups of 256 threads, 4 nonzeros each"""
    return n_cu * 16 * 256 * STREAM_CHUNK


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _triplet(indptr, indices, values):
    return np.asarray(indptr, dtype=np.uint64), np.asarray(indices, dtype=np.uint32), np.asarray(values, dtype=np.uint32)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def outer_ids(n_outer, indptr):
    return np.repeat(np.arange(n_outer, dtype=np.int64), np.diff(np.asarray(indptr, dtype=np.int64)))


def transpose(n_outer, n_inner, indptr, indices, values):
    """The n_inner x n_outer copy: a stable argsort on the inner index (outer ids ascend inside each inner vector)."""
    indptr, indices, values = _triplet(indptr, indices, values)
    order = np.argsort(indices, kind="stable")
    tip = np.zeros(n_inner + 1, dtype=np.uint64)
    tip[1:] = np.cumsum(np.bincount(indices.astype(np.int64), minlength=n_inner)[:n_inner]) if n_inner else 0
    return tip, outer_ids(n_outer, indptr)[order].astype(np.uint32), values[order]


def validate(n_outer, n_inner, indptr, indices, values):
    """(violations, zeros, max). A violation is an indptr entry that decreases or exceeds the number of nonzeros; with a sound indptr,
    an index >= n_inner, or an index that is not above its predecessor in the same vector. Vector by vector."""
    indptr, indices, values = _triplet(indptr, indices, values)
    nnz = indices.shape[0]
    ip = [int(x) for x in indptr]
    zeros = int(np.count_nonzero(values == 0))
    largest = int(values.max()) if nnz else 0
    bad = sum(1 for o in range(n_outer) if ip[o + 1] < ip[o] or ip[o + 1] > nnz)
    if bad or ip[0] != 0:
        return max(bad, 1), zeros, largest
    for o in range(n_outer):
        v = indices[ip[o]:ip[o + 1]].astype(np.int64)
        if v.shape[0]:
            bad += int(np.count_nonzero(v >= n_inner)) + int(np.count_nonzero(v[1:] <= v[:-1]))
    return bad, zeros, largest


def compact(n_outer, indptr, indices, values):
    """Stored zeros dropped."""
    indptr, indices, values = _triplet(indptr, indices, values)
    keep = values != 0
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint64)
    return before[indptr.astype(np.int64)], indices[keep], values[keep]


def sort_within(n_outer, indptr, indices, values):
    """Every outer vector sorted by index, its counts carried along."""
    indptr, indices, values = _triplet(indptr, indices, values)
    ix, vv = indices.copy(), values.copy()
    for o in range(n_outer):
        a, b = int(indptr[o]), int(indptr[o + 1])
        order = np.argsort(indices[a:b], kind="stable")
        ix[a:b], vv[a:b] = indices[a:b][order], values[a:b][order]
    return indptr.copy(), ix, vv


def items(indptr):
    """Work items per outer vector: one, or ceil(len / ITEM_NNZ) for a vector longer than ITEM_NNZ."""
    lens = np.diff(np.asarray(indptr, dtype=np.int64))
    return np.where(lens > ITEM_NNZ, -(-lens // ITEM_NNZ), 1)


def select_outer(n_outer, indptr, indices, values, idx):
    """Outer vector j of the result is outer vector idx[j]."""
    indptr, indices, values = _triplet(indptr, indices, values)
    idx = np.asarray(idx, dtype=np.int64)
    lens = (indptr[idx + 1] - indptr[idx]).astype(np.int64)
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    src = np.repeat(indptr[idx].astype(np.int64) - ip[:-1].astype(np.int64), lens) + np.arange(int(ip[-1]), dtype=np.int64)
    return ip, indices[src], values[src]


def select_inner(n_outer, n_inner, indptr, indices, values, idx):
    """Inner position j of the result is inner position idx[j] (any order, repeats allowed); the vectors stay sorted."""
    indptr, indices, values = _triplet(indptr, indices, values)
    idx = np.asarray(idx, dtype=np.int64)
    order = np.argsort(idx, kind="stable")
    lo = np.searchsorted(idx[order], indices.astype(np.int64), side="left")
    hi = np.searchsorted(idx[order], indices.astype(np.int64), side="right")
    reps = hi - lo
    src = np.repeat(np.arange(indices.shape[0], dtype=np.int64), reps)
    k = np.arange(src.shape[0], dtype=np.int64) - np.repeat(np.cumsum(reps) - reps, reps)
    new_pos = order[np.repeat(lo, reps) + k].astype(np.uint32)
    before = np.concatenate([[0], np.cumsum(reps)]).astype(np.uint64)
    return sort_within(n_outer, before[indptr.astype(np.int64)], new_pos, values[src])


def product(n_outer, indptr, indices, values, x):
    """out[o, :] = sum over the nonzeros of outer vector o of count * x[index, :], in u32: x is n_inner x l, u32."""
    indptr, indices, values = _triplet(indptr, indices, values)
    x = np.asarray(x, dtype=np.uint32)
    terms = values.astype(np.uint64)[:, None] * x[indices.astype(np.int64)].astype(np.uint64)  # wraps modulo 2^64, which keeps modulo 2^32
    run = np.concatenate([np.zeros((1, x.shape[1]), dtype=np.uint64), np.cumsum(terms, axis=0, dtype=np.uint64)])
    ip = indptr.astype(np.int64)
    return ((run[ip[1:]] - run[ip[:-1]]) & np.uint64(U32_MAX)).astype(np.uint32)


def product_t(n_outer, n_inner, indptr, indices, values, y):
    """out[i, :] = sum over the nonzeros at inner position i of count * y[outer id, :], in u32: y is n_outer x l, u32."""
    return product(n_inner, *transpose(n_outer, n_inner, indptr, indices, values), y)


def sums(n_outer, n_inner, indptr, indices, values):
    """(sum per outer vector, sum per inner position), u32."""
    one = np.ones((1, 1), dtype=np.uint32)
    return (product(n_outer, indptr, indices, values, np.ones((n_inner, 1), dtype=np.uint32))[:, 0],
            product_t(n_outer, n_inner, indptr, indices, values, np.repeat(one, n_outer, axis=0))[:, 0])


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def build(n_inner, lengths, rng, lo=1, hi=4):
    """A copy whose outer vectors have the given lengths (each <= n_inner): vector by vector the indices step through the whole inner
    range with a random offset inside every step, so they ascend strictly and nearly every vector start lies below the index before
    it. Counts are drawn from [lo, hi)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.max(initial=0) <= n_inner
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    nnz = int(indptr[-1])
    per = np.repeat(lengths, lengths)
    k = np.arange(nnz, dtype=np.int64) - np.repeat(indptr[:-1].astype(np.int64), lengths)
    step = n_inner // np.maximum(per, 1)
    indices = (k * step + np.floor(rng.random(nnz) * step).astype(np.int64)).astype(np.uint32)
    values = rng.integers(lo, hi, size=nnz, dtype=np.uint64).astype(np.uint32)
    return indptr, indices, values


def scattered_lengths(n_outer, n_full, rng, lo=1, hi=10):
    """n_full of the n_outer vectors hold lo .. hi - 1 nonzeros, the first and the last vector among them; the rest are empty."""
    lengths = np.zeros(n_outer, dtype=np.int64)
    at = rng.choice(n_outer, size=min(n_full, n_outer), replace=False)
    lengths[at] = rng.integers(lo, hi, size=at.shape[0])
    lengths[0], lengths[-1] = max(lengths[0], lo), max(lengths[-1], lo)
    return lengths


class Case:
    """One matrix: n_outer x n_inner and its read-only triplet."""

    def __init__(self, n_outer, n_inner, indptr, indices, values, **notes):
        self.n_outer, self.n_inner = int(n_outer), int(n_inner)
        self.indptr, self.indices, self.values = _freeze(*_triplet(indptr, indices, values))
        self.notes = notes

    @property
    def triplet(self):
        return self.indptr, self.indices, self.values

    @property
    def nnz(self):
        return int(self.indices.shape[0])

    @property
    def max_value(self):
        return int(self.values.max()) if self.nnz else 0

    def args(self):
        return (self.n_outer, self.n_inner) + self.triplet

    def with_arrays(self, indptr=None, indices=None, values=None, **notes):
        return Case(self.n_outer, self.n_inner, self.indptr if indptr is None else indptr, self.indices if indices is None else indices,
                    self.values if values is None else values, **dict(self.notes, **notes))


# ---- transposed copy: both sort routes --------------------------------------------------------------------------------------------
def _wide(n_outer, n_inner, big, seed, long_vector=0, n_full=600, lo=1, hi=10):
    """A few thousand nonzeros over n_outer x n_inner (n_full vectors of lo .. hi - 1), counts below 2^31, the corner positions (0, 0)
    and (last, last) stored, and the count `big` at a seeded place (None: none). long_vector: one outer vector in the middle with that
    many nonzeros."""
    rng = np.random.default_rng(seed)
    lengths = scattered_lengths(n_outer, n_full, rng, lo, hi)
    if long_vector:
        lengths[n_outer // 2] = long_vector
    ip, ix, vv = build(n_inner, lengths, rng, 1, 2**31)
    ix[0], ix[-1] = 0, n_inner - 1
    at = None
    if big is not None:
        at = int(rng.integers(0, vv.shape[0]))
        vv[at] = big
    return Case(n_outer, n_inner, ip, ix, vv, big_at=at)


# name -> (builder, bit sum, route). The three shapes' sums are 16 + 16 + 32, 17 + 16 + 32 and 17 + 17 + 32.
@functools.lru_cache(maxsize=None)
def transpose_case(name):
    if name == "edge_64":
        return _wide(65536, 65536, U32_MAX, 11)
    if name == "edge_64_small":           # the same edge below and above the sizes at which rocprim's radix sort changes its algorithm:
        return _wide(65536, 65536, U32_MAX, 16, n_full=120)              # one block (up to 1024 keys) ...
    if name == "edge_64_large":
        return _wide(65536, 65536, U32_MAX, 17, n_full=65536, lo=12, hi=23)  # ... and beyond the merge sort's 2^20 keys
    if name == "pair_65":
        return _wide(65536, 65537, U32_MAX, 12)
    if name == "pair_66":
        return _wide(65537, 65537, 2**31, 13)
    if name == "packed_65_small_counts":  # the 65-bit case, its counts all below 2^31: 31 bits of count
        return _wide(65536, 65537, None, 12)
    if name == "long_pair":               # one outer vector of 8193 nonzeros: two work items in pack_outer_kernel ...
        return _wide(65536, 65537, U32_MAX, 14, long_vector=ITEM_NNZ + 1)
    if name == "long_packed":             # ... and the same vector through pack_key_kernel
        return _wide(65536, 65537, None, 14, long_vector=ITEM_NNZ + 1)
    rng = np.random.default_rng(15)
    if name == "one_outer":
        return Case(1, 5000, *build(5000, [700], rng, 1, 2**20))
    if name == "one_inner":
        lengths = (rng.random(3000) < 0.4).astype(np.int64)
        return Case(3000, 1, *build(1, lengths, rng, 1, 2**20))
    if name == "all_ones":
        return Case(300, 200, *build(200, rng.integers(0, 21, size=300), rng, 1, 2))
    if name == "empty":
        return Case(40, 30, np.zeros(41, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32))
    if name == "mostly_empty_inner":      # every nonzero sits at one of 12 inner positions of 20000
        places = np.sort(rng.choice(20000, size=12, replace=False))
        hit = rng.random((500, 12)) < 0.5
        ip = np.concatenate([[0], np.cumsum(hit.sum(axis=1))])
        ix = np.broadcast_to(places, hit.shape)[hit]
        return Case(500, 20000, ip, ix, rng.integers(1, 2**16, size=ix.shape[0]))
    raise KeyError(name)


TRANSPOSE_CASES = {  # name -> (ib + ob + cb, route); None: the copy has no nonzeros and nothing is sorted
    "edge_64": (64, PACKED), "edge_64_small": (64, PACKED), "edge_64_large": (64, PACKED), "pair_65": (65, PAIR), "pair_66": (66, PAIR), "packed_65_small_counts": (64, PACKED),
    "long_pair": (65, PAIR), "long_packed": (64, PACKED),
    "one_outer": (13 + 1 + 20, PACKED), "one_inner": (1 + 12 + 20, PACKED), "all_ones": (8 + 9 + 1, PACKED), "empty": None,
    "mostly_empty_inner": (15 + 9 + 16, PACKED),
}


# ---- where the largest count is read ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def max_case(name):
    """300 x 4096, counts 1 .. 3 and one 2^32 - 1: at the last nonzero with nnz mod 4 = 1, 2, 3 (the last, partial chunk of four), or at
    nonzero 0."""
    rng = np.random.default_rng(21)
    lengths = rng.integers(0, 21, size=300)
    lengths[-1] = 7
    want = {"last_mod_1": 1, "last_mod_2": 2, "last_mod_3": 3, "first": 0}[name]
    lengths[-1] += (want - int(lengths.sum())) % 4
    ip, ix, vv = build(4096, lengths, rng, 1, 4)
    at = 0 if name == "first" else vv.shape[0] - 1
    vv[at] = U32_MAX
    return Case(300, 4096, ip, ix, vv, big_at=at)


MAX_CASES = ("last_mod_1", "last_mod_2", "last_mod_3", "first")


@functools.lru_cache(maxsize=None)
def big_case(n_cu):
    """4096 x 4096 with stream_span(n_cu) + 1029 nonzeros (about 4.2 M at 256 CUs): the last 1029 are the second trip of the
    grid-stride loop of validate_stream_kernel. Counts 1 .. 3 and one 2^32 - 1 in the middle of that second trip. Ten empty vectors in
    a run, the ten after them twice as long; the last eight vectors hold 100 nonzeros each."""
    rng = np.random.default_rng(22)
    n, nnz = 4096, stream_span(n_cu) + 1029
    lengths = np.full(n, nnz // n, dtype=np.int64)
    lengths[:nnz % n] += 1
    lengths[20:30] += lengths[10:20]
    lengths[10:20] = 0
    lengths[30:38] += lengths[-8:] - 100
    lengths[-8:] = 100  # several vector starts and ends inside the second trip
    ip, ix, vv = build(n, lengths, rng, 1, 4)
    at = stream_span(n_cu) + 515
    vv[at] = U32_MAX
    return Case(n, n, ip, ix, vv, big_at=at, second_trip=stream_span(n_cu))


# ---- validation -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def valid_base():
    """400 x 3000, a few thousand nonzeros; empty vectors scattered and in runs (40 .. 49, 200 .. 202 and the last five); vector 50
    behind the first run holds one nonzero, vector 203 behind the second holds five. nnz mod 4 = 2."""
    rng = np.random.default_rng(31)
    lengths = rng.integers(0, 19, size=400)
    lengths[rng.random(400) < 0.15] = 0
    lengths[40:50] = 0
    lengths[50] = 1
    lengths[51] = 6
    lengths[200:203] = 0
    lengths[203] = 5
    lengths[-5:] = 0
    lengths[-6] = 9
    lengths[-6] += (2 - int(lengths.sum())) % 4
    return Case(400, 3000, *build(3000, lengths, rng, 1, 1000))


VIOLATIONS = ("descent", "duplicate", "beyond", "indptr_decrease", "indptr_beyond")
PLACES = ("mod_0", "mod_1", "mod_2", "mod_3", "last", "after_empty_run")


def vector_of(indptr, p):
    return int(np.searchsorted(np.asarray(indptr, dtype=np.int64), p, side="right")) - 1


def place(case, violation, where):
    """The nonzero position a violation of that type goes to. Index violations inside a vector (descent, duplicate) need a
    predecessor in the same vector; an index of n_inner is exactly one violation only at the end of a vector; the indptr violations
    change the entry of the vector that starts at the position (never the last vector, so that a raised entry stays <= nnz).
    after_empty_run (valid_base only): vector 50, one nonzero directly behind the empty vectors 40 .. 49, or for the violations that
    need a predecessor the second nonzero of vector 203, behind the empty vectors 200 .. 202."""
    ip = case.indptr.astype(np.int64)
    full = np.diff(ip) > 0
    starts, ends = ip[:-1][full], ip[1:][full] - 1
    nnz = case.nnz
    if violation in ("descent", "duplicate"):
        ok = np.setdiff1d(np.arange(1, nnz), starts)
    elif violation == "beyond":
        ok = ends
    else:
        ok = starts[1:-1]
    if where == "second_trip":
        return int(ok[ok >= case.notes["second_trip"] + 100][0])
    if where == "last":
        return int(ok[-1])
    if where == "after_empty_run":
        assert case is valid_base() and ip[50] == ip[40] and ip[51] - ip[50] == 1 and ip[203] == ip[200] and ip[204] - ip[203] >= 2
        return int(ip[203]) + 1 if violation in ("descent", "duplicate") else int(ip[50])
    r = int(where[-1])
    mid = ok[ok >= nnz // 3]
    return int(mid[mid % 4 == r][0])


def violate(case, violation, p):
    """The case with exactly one violation of that type at nonzero position p (see `place`). The two indptr violations break one and
    two entries: the vector that starts at p ends before it starts, and with nnz + 1 the vector before it ends beyond the nonzeros."""
    ip, ix = case.indptr.copy(), case.indices.copy()
    if violation == "descent":
        ix[p - 1], ix[p] = ix[p], ix[p - 1]
    elif violation == "duplicate":
        ix[p] = ix[p - 1]
    elif violation == "beyond":
        ix[p] = case.n_inner
    else:
        o = vector_of(ip, p)  # the non-empty vector that starts at p
        ip[o] = int(ip[o + 1]) + 1 if violation == "indptr_decrease" else case.nnz + 1
    return case.with_arrays(indptr=ip, indices=ix)


def start_descent_places(case):
    """Vector starts p > 0 whose index does not lie above the index before them (no violation: another vector), one per residue of the
    chunk of four, the start behind the run of empty vectors, and the last vector start."""
    ip = case.indptr.astype(np.int64)
    starts = ip[:-1][np.diff(ip) > 0]
    starts = starts[starts > 0]
    down = starts[case.indices[starts] <= case.indices[starts - 1]]
    out = {f"mod_{r}": int(down[down % 4 == r][len(down) // 8]) for r in range(4)}
    out["last"] = int(down[-1])
    if case is valid_base():
        out["after_empty_run"] = int(ip[50])
    return out


def equal_across_a_start(case):
    """(case, places): the index of vectors of one nonzero set to the index before them, the last index of the vector before. Equal
    indices in two vectors are no violation. One such vector per residue of its position, as far as the case has them."""
    ip = case.indptr.astype(np.int64)
    single = ip[:-1][np.diff(ip) == 1]
    single = single[single > 0]
    places = [int(single[single % 4 == r][0]) for r in range(4) if np.any(single % 4 == r)]
    ix = case.indices.copy()
    for p in places:
        ix[p] = ix[p - 1]
    return case.with_arrays(indices=ix), places


@functools.lru_cache(maxsize=None)
def all_starts_descend():
    """257 vectors of 3 .. 9 nonzeros, each starting below the end of the one before."""
    rng = np.random.default_rng(32)
    c = Case(257, 900, *build(900, rng.integers(3, 10, size=257), rng, 1, 50))
    ip = c.indptr.astype(np.int64)
    assert np.all(c.indices[ip[1:-1]] <= c.indices[ip[1:-1] - 1])
    return c


# ---- stored zeros -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def zeros_case(name):
    """300 x 2000 with stored zeros: "residues": at positions of every residue of the chunk of four, the first and the last nonzero
    among them; "vector": one vector of only zeros besides; "all": every count zero; "with_max": zeros and one 2^32 - 1."""
    rng = np.random.default_rng(41)
    lengths = rng.integers(0, 21, size=300)
    lengths[0], lengths[-1], lengths[100] = 3, 4, 12
    ip, ix, vv = build(2000, lengths, rng, 1, 9)
    nnz = vv.shape[0]
    if name == "all":
        vv[:] = 0
    else:
        at = np.concatenate([[0, nnz - 1], 400 + 5 * np.arange(40), 1000 + np.arange(9)])  # 400 + 5 k: residues 0, 1, 2, 3 in turn
        vv[at] = 0
        if name == "vector":
            vv[int(ip[100]):int(ip[101])] = 0
        if name == "with_max":
            vv[999], vv[1009] = U32_MAX, U32_MAX  # on either side of a run of nine zeros
    return Case(300, 2000, ip, ix, vv)


ZEROS_CASES = ("residues", "vector", "all", "with_max")


# ---- unsorted input ---------------------------------------------------------------------------------------------------------------
UNSORTED_LENGTHS = (0, 1, ITEM_NNZ, 0, 0, ITEM_NNZ + 1, 20000, 1, 0)


@functools.lru_cache(maxsize=None)
def unsorted_case(zeros=False):
    """n_inner = 70001, vectors of UNSORTED_LENGTHS nonzeros, the indices of every vector in a seeded shuffle."""
    rng = np.random.default_rng(51)
    ip, ix, vv = build(70001, UNSORTED_LENGTHS, rng, 1, 2**32)
    for o in range(len(UNSORTED_LENGTHS)):
        a, b = int(ip[o]), int(ip[o + 1])
        order = rng.permutation(b - a)
        ix[a:b], vv[a:b] = ix[a:b][order], vv[a:b][order]
    if zeros:
        vv[rng.choice(vv.shape[0], size=500, replace=False)] = 0
    return Case(len(UNSORTED_LENGTHS), 70001, ip, ix, vv)


# ---- work items -------------------------------------------------------------------------------------------------------------------
ITEM_LENGTHS = (0, 1, ITEM_NNZ - 1, ITEM_NNZ, ITEM_NNZ + 1, 2 * ITEM_NNZ, 2 * ITEM_NNZ + 1, 3 * ITEM_NNZ + 1, 0)


@functools.lru_cache(maxsize=None)
def items_case():
    """Vectors of ITEM_LENGTHS nonzeros over 30011 inner positions, counts in [2^30, 2^32): every u32 sum wraps."""
    rng = np.random.default_rng(61)
    return Case(len(ITEM_LENGTHS), 30011, *build(30011, ITEM_LENGTHS, rng, 2**30, 2**32))


# ---- AdaptiveVec tables for the decoder (made by the oracle, never by the device encoder) -------------------------------------------
DECODE_LENGTHS = ag.LENGTHS + (42, 2048, 2049, 4097)  # + two Dense3 words exactly; the 2048-unit chunk and one beyond; two chunks and one
DECODE_CHUNK = 2048                                   # units per workgroup of decode_kernel
THRESHOLD = {"D3": 7, "D4": 15, "D8": 255, "D16": 65535, "S3": 7, "S4": 15, "S8": 255}


@functools.lru_cache(maxsize=None)
def decode_grid():
    """{length: 25 (indices, values)}: adaptive_grid's vectors, and the same 5 densities x 5 ranges at the further lengths."""
    out = dict(ag.grid())
    rng = np.random.default_rng(71)
    for length in DECODE_LENGTHS[len(ag.LENGTHS):]:
        vecs = []
        for dens in ag.DENSITIES:
            for lo, hi in ag.RANGES:
                n = min(length, int(round(length * dens)))
                idx = np.sort(rng.choice(length, size=n, replace=False)).astype(np.uint32)
                val = rng.integers(lo, hi, size=n).astype(np.uint32)
                tail = rng.random(n) < 0.05
                val[tail] = rng.integers(1, 100000, size=int(tail.sum())).astype(np.uint32)
                vecs.append((idx, val))
        out[length] = vecs
    return out


def decoded(vecs):
    """The triplet the oracle's iter() gives for a list of AdaptiveVec: what the device decoder has to return."""
    parts = [v.iter() for v in vecs]
    ip = np.concatenate([[0], np.cumsum([len(p) for p, _ in parts])]).astype(np.uint64)
    cat = lambda k: np.concatenate([p[k] for p in parts]).astype(np.uint32) if parts else np.zeros(0, dtype=np.uint32)  # noqa: E731
    return ip, cat(0), cat(1)


def _random_vec(kind, length, density, rng, lo=1, hi=100000):
    n = int(round(length * density))
    idx = np.sort(rng.choice(length, size=n, replace=False)).astype(np.uint32)
    return av.AdaptiveVec.with_kind(kind, length, rng.integers(lo, hi, size=n).astype(np.uint32), idx)


MIXED_LENGTH = 70001


@functools.lru_cache(maxsize=None)
def mixed_table():
    """One table at length 70001: the eight kinds in a seeded order, each spanning several chunks of 2048 units; empty vectors (of
    kinds that own no chunk, V / S3 / S8, and of dense kinds, whose chunks hold nothing) first, last and in runs between them; one D16
    vector whose only nonzeros lie in its last chunk. Returns (list of AdaptiveVec, note per vector)."""
    rng = np.random.default_rng(72)
    n = MIXED_LENGTH
    empty = np.zeros(0, dtype=np.uint32)
    e = lambda kind: (av.AdaptiveVec.with_kind(kind, n, empty, empty), "empty " + kind)  # noqa: E731
    density = {"D3": 0.3, "D4": 0.3, "D8": 1.0, "D16": 0.05, "V": 0.3, "S3": 1.0, "S4": 0.2, "S8": 0.15}
    order = [av.KINDS[i] for i in rng.permutation(8)]
    full = [(_random_vec(k, n, density[k], rng), k) for k in order]
    last_chunk = (n - 1) // DECODE_CHUNK * DECODE_CHUNK
    tail_idx = np.sort(rng.choice(np.arange(last_chunk, n), size=90, replace=False)).astype(np.uint32)
    tail = (av.AdaptiveVec.with_kind("D16", n, rng.integers(1, 100000, size=90).astype(np.uint32), tail_idx), "last chunk only")
    table = [e("V"), e("S3"), full[0], e("S8"), e("V"), e("D3"), full[1], full[2], e("V"), tail, e("S4"), e("D4"), e("V"), full[3],
             full[4], e("S8"), full[5], e("D16"), e("V"), full[6], full[7], e("S3"), e("V")]
    return [v for v, _ in table], [note for _, note in table]


def _drop_fallback(v, which):
    d = v.dense
    d.fallback_indexes, d.fallback_values = np.delete(d.fallback_indexes, which), np.delete(d.fallback_values, which)
    return v


@functools.lru_cache(maxsize=None)
def foreign_vectors(length=5000):
    """Vectors the encoder never emits but the reference decodes, one list per encoding that can express them: (name, AdaptiveVec).
    stored zeros: a V entry with value 0, an S* entry whose field is 0 (both skipped); orphan: fields at the fallback threshold
    whose fallback entry is gone (SimpleSparse::get gives 0: nothing there); only orphans: a vector of nothing else (empty)."""
    rng = np.random.default_rng(73)
    out = []
    idx = np.sort(rng.choice(length, size=700, replace=False)).astype(np.uint32)
    val = rng.integers(1, 100000, size=700).astype(np.uint32)
    val[::3] = 0  # every third stored entry, the first included
    val[-1] = 0
    for kind in ("V", "S3", "S4", "S8"):
        out.append(("stored zeros " + kind, av.AdaptiveVec.with_kind(kind, length, val, idx)))
    out.append(("only stored zeros V", av.AdaptiveVec.with_kind("V", length, np.zeros(5, dtype=np.uint32), idx[:5])))
    out.append(("only stored zeros S4", av.AdaptiveVec.with_kind("S4", length, np.zeros(300, dtype=np.uint32), idx[:300])))
    for kind, th in THRESHOLD.items():
        v = rng.integers(1, 2 * th + 2, size=700).astype(np.uint32)  # about half reach the threshold
        v[[0, 350, 699]] = th + 5
        a = av.AdaptiveVec.with_kind(kind, length, v, idx)
        n_fb = a.dense.fallback_indexes.shape[0]
        out.append(("orphan " + kind, _drop_fallback(a, [0, n_fb // 2, n_fb - 1])))  # the first, a middle and the last fallback entry
        b = av.AdaptiveVec.with_kind(kind, length, np.full(700, th, dtype=np.uint32), idx)
        out.append(("only orphans " + kind, _drop_fallback(b, np.arange(700))))
    return out
