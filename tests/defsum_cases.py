"""Inputs and the third opinion for the device DefSumModel (k13_defsum_model.hip, BWTC levels 1-5 of the batched compress).

* model(): a plain restatement of the ENCODE side of the reference's lib/DefSumModel.js (constructor :11-24, _update :39-80,
  encode :94-111) that also counts what a row of symbols reaches: triples, escapes, escapes of a symbol seen before, and the escape
  symbol's updates refused by the cap of 40 (:42) and by the `updateThresh - 1` rule (:46).
* rows(): the symbol rows the model is run on alone (cjs_dbg_defsum_triples): every length and alphabet at which the kernel takes
  another path (a chunk is 64 symbols, the first 88 symbols of a block all escape, the cap refuses after 40 of them), and three
  families that reach the rare branches.  check_families() ASSERTS that they do, on the CPU: a family that silently stops reaching
  a branch fails there, not on the GPU.
* golden_docs(): the documents of tests/golden/golden_bwtc_defsum.json (reference-made digests, make_golden_bwtc_defsum.py), chosen
  so that the MODEL's input - after BWT and MTF - is hostile.  Everything is a pure function of a seed."""
import numpy as np

MAX_ESCAPE_COUNT = 40                                     # lib/DefSumModel.js:9
PROB_TOTAL = 256                                          # :8

NSYMS = [0, 1, 2, 63, 64, 65, 87, 88, 89, 127, 128, 129, 255, 256, 257, 1000, 4096]
ALPHAS = [1, 2, 3, 17, 255, 256]


def model(sym, alpha):
    """-> (triples [(sy_f, lt_f, tot_f)], counts dict).  Symbols in [0, alpha]; DefSumModel(coder, alpha + 1) (lib/BWTC.js:107)."""
    size = alpha + 1
    ESC = size                                            # :14
    prob = [0] * (size + 2)                               # :16
    escape = list(range(size + 1))                        # :17, :20-22
    update = [0] * (size + 1)                             # :18
    prob[ESC + 1] = PROB_TOTAL                            # :19
    st = dict(uc=0, th=PROB_TOTAL - PROB_TOTAL // 2, epoch=0)     # :23-24
    cnt = dict(triples=0, escapes=0, re_escapes=0, cap_refused=0, cap_refused_late=0, thresh_refused=0, rebuilds=0)
    seen = set()
    out = []

    def _update(s):                                       # :39-80
        if s == ESC:
            if update[s] >= MAX_ESCAPE_COUNT:             # :42
                cnt["cap_refused"] += 1
                cnt["cap_refused_late"] += st["epoch"] > 0
                return
            if st["uc"] >= st["th"] - 1:                  # :46
                cnt["thresh_refused"] += 1
                return
        update[s] += 1                                    # :48-49
        st["uc"] += 1
        if st["uc"] < st["th"]:                           # :51
            return
        cum = cum_esc = odd = 0                           # :55
        for i in range(size + 1):                         # :56-70
            new = ((prob[i + 1] - prob[i]) >> 1) + update[i]
            prob[i] = cum
            escape[i] = cum_esc
            if new:
                cum += new
                odd += new & 1
            else:
                cum_esc += 1
        prob[size + 1] = cum                              # :71
        assert cum == PROB_TOTAL                          # :72
        st["th"] = PROB_TOTAL - (cum - odd) // 2          # :74
        for i in range(size + 1):                         # :76-78
            update[i] = 0
        update[ESC] = 1                                   # :79
        st["uc"] = 1                                      # :80
        st["epoch"] += 1
        cnt["rebuilds"] += 1

    def encode(s):                                        # :94-111
        lt = prob[s]
        sy = prob[s + 1] - lt
        if sy:
            out.append((sy, lt, PROB_TOTAL))              # encodeShift(sy_f, lt_f, 8) == encodeFreq(sy_f, lt_f, 256)
            return _update(s)
        assert s != ESC                                   # :103
        cnt["escapes"] += 1
        cnt["re_escapes"] += s in seen
        encode(ESC)                                       # :104
        lt = escape[s]                                    # :106-109
        out.append((escape[s + 1] - lt, lt, escape[ESC]))
        return _update(s)

    for s in sym:
        s = int(s)
        assert 0 <= s <= alpha
        encode(s)
        seen.add(s)
    cnt["triples"] = len(out)
    return out, cnt


def words(triples):
    """the layout of K10 / K13: sylt[k] = sy_f | lt_f << 16, tot[k] = tot_f"""
    a = np.array([sy | (lt << 16) for sy, lt, _ in triples], dtype=np.uint32)
    t = np.array([to for _, _, to in triples], dtype=np.uint32)
    return a, t


# ---- the families --------------------------------------------------------------------------------------------------------
def zipf_row(seed, n=4096, alpha=256):
    """a few very common symbols and a long tail: symbols come back after the halvings took them to 0 (re-escapes), and an escape
    meets updateCount == updateThresh - 1 now and then"""
    rng = np.random.RandomState(seed)
    return np.minimum(rng.zipf(1.3, size=n) - 1, alpha).astype(np.uint16)


def sorted_row(seed, n=4096, alpha=256):
    """every symbol in one run of ~16: almost every symbol escapes (close to two triples a symbol), the cap of 40 refuses in
    every epoch"""
    rng = np.random.RandomState(seed)
    return np.sort(rng.randint(0, alpha + 1, size=n)).astype(np.uint16)


def fresh_row(seed, n=4096, alpha=256):
    """three common symbols and a rare one every ~25: the rare ones are halved away before they return"""
    rng = np.random.RandomState(seed)
    out = rng.randint(0, 3, size=n).astype(np.uint16)
    p = int(rng.randint(5, 25))
    while p < n:
        out[p] = int(rng.randint(3, alpha + 1))
        p += int(rng.randint(15, 36))
    return out


ZIPF_SEEDS = (1, 2, 3)
SORTED_SEED = 4
FRESH_SEED = 5


def family_rows():
    """-> [(name, symbols uint16, alpha)]"""
    return ([("zipf%d" % s, zipf_row(s), 256) for s in ZIPF_SEEDS] + [("sorted", sorted_row(SORTED_SEED), 256),
            ("fresh", fresh_row(FRESH_SEED), 256)])


def shape_rows():
    """uniform symbols in [0, alpha] at every length x alphabet, and all-zero rows (RUNA only)"""
    out = []
    for n in NSYMS:
        for a in ALPHAS:
            rng = np.random.RandomState(100000 + 300 * n + a)
            out.append(("u%d_a%d" % (n, a), rng.randint(0, a + 1, size=n).astype(np.uint16), a))
    for n, a in ((1, 1), (64, 1), (88, 3), (129, 17), (1000, 256), (4096, 256)):
        out.append(("zero%d_a%d" % (n, a), np.zeros(n, np.uint16), a))
    return out


_ROWS = None


def rows():
    """-> [(name, symbols, alpha, sylt words, tot words, counts)], the restatement's answer included; computed once"""
    global _ROWS
    if _ROWS is None:
        _ROWS = []
        for name, s, a in family_rows() + shape_rows():
            tri, cnt = model(s, a)
            _ROWS.append((name, s, a) + words(tri) + (cnt,))
    return _ROWS


def check_families():
    """the conditions the rows must reach (asserted; the seeds were chosen with this restatement, not by running the kernel)"""
    R = {r[0]: r for r in rows()}
    fam = [R[n] for n, _, _ in family_rows()]
    assert any(r[5]["thresh_refused"] >= 1 for r in fam), [r[5] for r in fam]
    assert any(r[5]["cap_refused_late"] >= 1 for r in fam)
    assert any(r[5]["re_escapes"] >= 100 for r in fam)
    assert any(r[5]["triples"] >= 1.8 * r[1].size for r in fam)
    for r in rows():
        assert r[5]["triples"] <= 2 * r[1].size and r[5]["triples"] == r[1].size + r[5]["escapes"], r[0]
    # every block's first 88 symbols all escape, and after 40 of them the cap refuses the escape symbol's update
    c = R["u88_a256"][5]
    assert c["escapes"] == 88 and c["cap_refused"] == 48 and c["rebuilds"] == 1, c
    assert R["u87_a256"][5]["rebuilds"] == 0
    return {r[0]: r[5] for r in fam}


def pack_rows(sel):
    """rows -> (sym [nb * stride] uint16, nsym, alpha, stride): stride = the longest row rounded up to 4 (at least 4)"""
    stride = max(4, (max(r[1].size for r in sel) + 3) & ~3)
    sym = np.zeros(len(sel) * stride, np.uint16)
    for k, r in enumerate(sel):
        sym[k * stride:k * stride + r[1].size] = r[1]
    nsym = np.array([r[1].size for r in sel], dtype=np.uint32)
    alpha = np.array([r[2] for r in sel], dtype=np.uint32)
    return sym, nsym, alpha, stride


def run_model(L, sel, on_host):
    """cjs_dbg_defsum_triples over the rows -> [(ntri, sylt words, tot words)]; ostride is exactly 2 * stride"""
    sym, nsym, alpha, stride = pack_rows(sel)
    nb, ostride = len(sel), 2 * stride
    sylt = np.full(nb * ostride, 0xDDDDDDDD, np.uint32)
    tot = np.full(nb * ostride, 0xDDDDDDDD, np.uint32)
    ntri = np.full(nb, 0xDDDDDDDD, np.uint32)
    rc = L.cjs_dbg_defsum_triples(sym.ctypes.data, nsym.ctypes.data, alpha.ctypes.data, nb, stride, sylt.ctypes.data, tot.ctypes.data,
                                  ntri.ctypes.data, ostride, int(on_host))
    assert rc == 0, rc
    out = []
    for k in range(nb):
        n = int(ntri[k])
        assert n <= ostride, (sel[k][0], n)
        out.append((n, sylt[k * ostride:k * ostride + n].copy(), tot[k * ostride:k * ostride + n].copy()))
    return out


def assert_rows_equal(got, sel, what):
    for (n, a, t), r in zip(got, sel):
        assert n == r[5]["triples"], (what, r[0], n, r[5]["triples"])
        bad = np.nonzero((a != r[3]) | (t != r[4]))[0]
        assert bad.size == 0, (what, r[0], int(bad[0]), hex(int(a[bad[0]])), hex(int(r[3][bad[0]])), int(t[bad[0]]), int(r[4][bad[0]]))


def seventy():
    """70 rows of different lengths for one launch: the families, the longest shapes and a spread of the short ones"""
    R = rows()
    short = [r for r in R[5:] if r[1].size < 1000]
    sel = R[:5] + [r for r in R[5:] if r[1].size >= 1000] + short[::2] + short[1::2]
    return sel[:70]


# ---- documents of golden_bwtc_defsum.json ------------------------------------------------------------------------------------
def _sweeps(rng, n):
    """mostly two symbols, every ~1200 bytes a sweep over rarely used ones (tests/golden/bwtc_cases.py's _gap_heavy, a seed of its own)"""
    out = rng.randint(97, 99, size=n).astype(np.uint8)
    rare = np.arange(130, 250, dtype=np.uint8)
    p = 700
    while p + rare.size < n:
        k = int(rng.randint(8, rare.size))
        out[p:p + k] = rng.permutation(rare)[:k]
        p += int(rng.randint(900, 1700))
    return out


N_DOCS = 40
BIG_ID, BIG_LEVEL, BIG_LEN = "text100001_l1", 1, 100001


def doc(i):
    """-> (data uint8, level); levels 1-5, at most 30 000 bytes"""
    rng = np.random.RandomState(52000 + i)
    level = 1 + i % 5
    style = (i // 5) % 8
    n = int(rng.choice([300, 2000, 9000, 30000]))
    if style == 0:
        d = rng.randint(0, 256, size=n)                                       # uniform: a wide, near-flat index distribution
    elif style == 1:
        d = np.sort(rng.randint(0, 256, size=n))                              # sorted: zero runs, every symbol new once
    elif style == 2:
        d = _sweeps(rng, max(n, 4000))
    elif style == 3:
        d = rng.randint(0, 2, size=n) * 255                                   # two symbols
    elif style == 4:
        d = rng.choice(np.array([7, 8, 200]), size=n, p=[0.7, 0.2, 0.1])      # three symbols
    elif style == 5:
        k = max(1, n // 40)
        d = np.repeat(rng.randint(0, 256, size=k), rng.randint(1, 80, size=k))[:n]     # runs
    elif style == 6:
        d = np.concatenate([rng.randint(0, 256, size=n // 3 + 1), np.zeros(n // 3 + 1, np.int64), rng.randint(0, 3, size=n // 3)])   # flat, then runs, then tiny
    else:
        d = np.minimum(rng.zipf(1.3, size=n) - 1, 255)                        # a long tail
    return np.ascontiguousarray(d, dtype=np.uint8), level


def big_doc():
    """a full level-1 block and a block of one byte: the coder state of the document crosses two k11_code launches with 2 blocks in flight"""
    from compressjs_amd import synth
    return synth.text_like(BIG_LEN, 9)
