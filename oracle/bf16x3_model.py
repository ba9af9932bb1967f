"""numpy model of the three-way bfloat16 product of csrc/gemm.h ("X3") and the operands that make its terms visible
(tests/test_bf16x3_model.py, tests/test_gpu_gemm_edges.py).  Test infrastructure only, numpy only.

* `bf16`: round-to-nearest-even onto the upper 16 bits of the float32 pattern; `split3`: x -> h = bf16(x), m = bf16(x - h),
  l = bf16(x - h - m) as float32 arrays - `gemm_split3` of the kernel.
* `x3_product`: sum over a list of piece pairs, default the kernel's six, hh + (hm + mh) + (mm + hl + lh); with exact
  (float64) sums (`group=None`), or with the kernel's levels of float32 sums: `group` contraction indices are added exactly and
  rounded into the float32 accumulator, once per group and term in the kernel's order of terms; blocks of 512 are added into
  a second float32 sum, slices of 16 384 in float64.  `group=16` is one rounding per v_mfma_f32_32x32x16_bf16; `group=8`
  (`MFMA_GROUP`) is what the MI355X does - two groups of eight per instruction: with it the model reproduces 97 % of the
  elements of a 128 x 128 x 128 product of the device bit for bit, 78 % at K = 512, and every signed mean error; with 16, 24 %
  and 0.1 %.  The finer rounding matters for the operands below: a small term of a group of eight is ~0.8 units in the last
  place of an accumulator between 512 and 1024 and always rounds up to one, a bias of up to +1.8e-6 over a block of 512
  products where the model with 16 has noise of 3e-7.
* `piece_operands`: every element x = h + m + l with h = 1 + i / 128 (i < 32), m = (192 + j) 2^-16 (j < 64),
  l = (32 + k) 2^-23 (k < 32): x is a float32, split3 gives back exactly these pieces, and all of them are positive - a product
  term left out is a bias of ~K m m or ~K h l in every element instead of noise with random signs.
* `MUTATIONS`: the six single-term deletions and the pairing of al with bl instead of bh.
* `X3_SHAPES`, `X3_GRAM_SHAPES`: the shapes of the X3 test on the device; `BAR`: the project's float32 bar.
* `device_calls`: the calls of `Handle.gemm` that test makes, in the parent process and in its child without X3.
"""
import numpy as np

BAR = 2e-6                       # error / max(|A| @ |B|) of a float32 product (tests/test_gpu_kernels.py)
MFMA_GROUP, FLUSH, SLICE = 8, 512, 16384

# the kernel's terms in its order (small terms first): (piece of A, piece of B)
TERMS = (("l", "h"), ("h", "l"), ("m", "m"), ("m", "h"), ("h", "m"), ("h", "h"))
MUTATIONS = {("drop_" + a + b): tuple(t for t in TERMS if t != (a, b)) for a, b in TERMS}
MUTATIONS["al_bl_for_al_bh"] = (("l", "l"),) + TERMS[1:]

# (M, N, K) of the general products and (T, K) of the Gram products X X^T
X3_SHAPES = [(37, 53, 29), (33, 65, 64), (128, 128, 512), (128, 128, 544), (5, 7, 16384)]
X3_GRAM_SHAPES = [(129, 64), (129, 544)]


def bf16(x):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def split3(x):
    x = np.asarray(x, dtype=np.float32)
    h = bf16(x)
    r = x - h                    # exact in float32
    m = bf16(r)
    return h, m, bf16(r - m)


def piece_operands(shape, seed):
    """float32 array of `shape` whose elements have the known, positive pieces of the module docstring"""
    rng = np.random.default_rng(seed)
    h = 1.0 + rng.integers(0, 32, shape) / 128.0
    m = (192 + rng.integers(0, 64, shape)) * 2.0 ** -16
    l = (32 + rng.integers(0, 32, shape)) * 2.0 ** -23
    x64 = h + m + l
    x = x64.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), x64)
    gh, gm, gl = split3(x)
    assert np.array_equal(gh, h) and np.array_equal(gm, m) and np.array_equal(gl, l)
    return x


def x3_product(A, B, terms=TERMS, group=None):
    """A (M, K) @ B (K, N), float32 operands, as the sum of the listed products of bfloat16 pieces -> float64 (M, N);
    group: None (exact sums) or the number of products rounded into the float32 accumulator at a time (8 or 16)"""
    pa = dict(zip("hml", (p.astype(np.float64) for p in split3(A))))
    pb = dict(zip("hml", (p.astype(np.float64) for p in split3(B))))
    M, K = A.shape
    N = B.shape[1]
    if group is None:
        return sum(pa[a] @ pb[b] for a, b in terms)
    pad = -K % 16                # the kernel fills a partial k-tile with zeros
    steps, per = (K + pad) // 16, 16 // group
    sums = []                    # per term: (steps * per, M, N) exact sums of `group` products
    for a, b in terms:
        x = np.pad(pa[a], ((0, 0), (0, pad))).reshape(M, steps * per, group)
        y = np.pad(pb[b], ((0, pad), (0, 0))).reshape(steps * per, group, N)
        sums.append(np.einsum("msk,skn->smn", x, y))
    total = np.zeros((M, N))
    acc = np.zeros((M, N), dtype=np.float32)
    wide = np.zeros((M, N), dtype=np.float32)
    for s in range(steps):       # one MFMA per term and 16 contraction indices
        for t in sums:
            for g in range(per):
                acc = (acc.astype(np.float64) + t[s * per + g]).astype(np.float32)
        done = (s + 1) * 16
        if done % FLUSH == 0:
            wide = wide + acc
            acc = np.zeros((M, N), dtype=np.float32)
        if done % SLICE == 0 or s == steps - 1:
            total += acc.astype(np.float64) + wide.astype(np.float64)
            acc = np.zeros((M, N), dtype=np.float32)
            wide = np.zeros((M, N), dtype=np.float32)
    return total


def reference(A, B):
    """(float64 product, max of |A| @ |B|): what every comparison is against and relative to"""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    return A64 @ B64, float((np.abs(A64) @ np.abs(B64)).max())


def error(C, A, B):
    ref, scale = reference(A, B)
    return float(np.max(np.abs(C - ref))) / scale


def x3_operands(shape, gram=False):
    """the operands of one X3 case, A (M, K) and B (K, N): `shape` = (M, N, K), or (T, K) with gram (B = A^T)"""
    if gram:
        T, K = shape
        A = piece_operands((T, K), 1000 * T + K)
        return A, np.ascontiguousarray(A.T)
    M, N, K = shape
    return piece_operands((M, K), 1000 * M + K), piece_operands((K, N), 1000 * N + K + 1)


def case_id(shape, gram=False):
    return ("gram-" if gram else "") + "x".join(map(str, shape))


def device_calls():
    """(key, A as stored, B as stored, keyword arguments of Handle.gemm, A (M, K), B (K, N)) of every X3 product of the device
    test: A contiguous along the contraction, B in both orientations, and the Gram form; one slice (the flush levels are
    reached as the shapes name them) and the heuristic split count"""
    for shape in X3_SHAPES:
        A, B = x3_operands(shape)
        for b_nfast in (True, False):
            Bs = B if b_nfast else np.ascontiguousarray(B.T)
            for splits in (1, 0):
                yield ("%s-bn%d-s%d" % (case_id(shape), b_nfast, splits), A, Bs,
                       dict(a_kfast=True, b_nfast=b_nfast, splits=splits), A, B)
    for shape in X3_GRAM_SHAPES:
        A, B = x3_operands(shape, gram=True)
        for splits in (1, 0):
            yield ("%s-s%d" % (case_id(shape, True), splits), A, A,
                   dict(a_kfast=True, b_nfast=False, upper_only=True, mirror=1, splits=splits), A, B)
