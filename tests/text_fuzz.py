"""Adversarial PAF texts for the tests that go from text to written rows (tests/test_text_fuzz_cpu.py, tests/test_gpu_text_fuzz.py):
the intervals of tests/test_fuzz.py's make_batch (containment, equal starts, duplicates, records of a few bases, both strands) as
PAF rows whose cs tag consumes exactly the query span, in short operations: ':' runs of mostly 1 - 3 bases, substitutions, long
and short indels right beside them, leading zeros.  Text number i of a kind follows from (SEED, kind, i) alone; nothing here comes
from the product.  expected() is the whole reference pipeline on the oracle side."""
import collections
import functools
import random

SEED = 20261017
STYLES = (0, 1, 2)
RUNS = ((10000, False), (3, True))                                   # (K, non_skip_linkable) of every text
LETTERS = "acgtn"
INS, DEL = (1, 2, 5, 9, 70), (1, 2, 5, 64, 130)
# The share of an unshaped text's records whose tag is shaped all the same; the other tags may start or end with any operation.
# One rejected element rejects the whole run, and a text has about 75 records: with every tag unshaped (share 0) the oracle rejects
# 64 of the 72 runs of the first 36 texts and accepts 8, fewer than the quarter that must come out as files.  At 0.6 it rejects 35
# (71 elements) and accepts 37, so both kinds of run are well represented (counted on the oracle alone).
SHAPED_SHARE = 0.6
REFS = ("chrA", "chr2", "scaffold_3|x")


def _letters(rng, n):
    return "".join(rng.choice(LETTERS) for _ in range(n))


def _run(rng, n):
    """':n', 4 % with leading zeros."""
    return ":" + ("0" * rng.randrange(1, 4) if rng.random() < 0.04 else "") + str(n)


def random_tag(rng, n_qry, shaped):
    """A short-form cs tag that consumes exactly n_qry query bases and holds at least one ':' run -> (tag, reference bases,
    matches, alignment length).  shaped: the first and the last operation are ':' runs of 1 - 3 bases, as an aligner emits them;
    else any operation may come first or last."""
    ops, q, r, mat, aln, has_run = [], 0, 0, 0, 0, False
    tail = 0
    if shaped:
        if n_qry <= 3:
            return "cs:Z:" + _run(rng, n_qry), n_qry, n_qry, n_qry
        head = rng.randrange(1, min(3, n_qry - 1) + 1)
        tail = rng.randrange(1, min(3, n_qry - head) + 1)
        ops.append(_run(rng, head)); q = r = mat = aln = head; has_run = True
    room = n_qry - tail                                              # the operations in between consume [q, room)
    while q < room or (not shaped and rng.random() < 0.15):
        left = room - q
        k = rng.random()
        if left == 0 or k < 0.18:                                    # a deletion: no query base
            n = rng.choice(DEL)
            ops.append("-" + _letters(rng, n)); r += n; aln += n
        elif k < 0.63 or (left == 1 and not has_run and not tail):
            n = min(left, rng.choice((1, 1, 1, 2, 2, 3, 3, 3, rng.randrange(4, 31))))
            ops.append(_run(rng, n)); q += n; r += n; mat += n; aln += n; has_run = True
        elif k < 0.82:
            ops.append("*" + _letters(rng, 2)); q += 1; r += 1; aln += 1
        else:
            n = min(left, rng.choice(INS))
            if n == left and not has_run and not tail:               # keep a base for the run every tag holds
                continue
            ops.append("+" + _letters(rng, n)); q += n; aln += n
        if q == room and not has_run and not tail:                   # (unreachable: the branches above keep a base)
            raise AssertionError("tag without a match run")
    if tail:
        ops.append(_run(rng, tail)); q += tail; r += tail; mat += tail; aln += tail
    assert q == n_qry
    return "cs:Z:" + "".join(ops), r, mat, aln


def intervals(rng, n_contigs, n_max, L, style):
    """make_batch's query intervals: per contig (qry_total, [(qs, qe closed)])."""
    out = []
    for _ in range(n_contigs):
        n, qt, recs = rng.randrange(1, n_max + 1), L + rng.randrange(0, 50), []
        for i in range(n):
            if style == 0:                                           # anything goes
                qs = rng.randrange(0, L - 2); qe = min(L - 1, qs + rng.randrange(1, max(2, L // 3)))
            elif style == 1:                                         # few distinct boundaries: duplicates, containment, equal starts
                qs = rng.randrange(0, 6) * (L // 8); qe = min(L - 1, qs + rng.randrange(1, 4) * (L // 8))
            else:                                                    # a chain with overlaps
                qs = min(L - 3, i * (L // (n + 1)) + rng.randrange(0, 5)); qe = min(L - 1, qs + rng.randrange(L // (n + 1), 2 * L // (n + 1) + 2))
            if rng.random() < 0.05:
                qe = qs + rng.randrange(0, 3)                        # a record of 1 - 3 bases
            recs.append((qs, max(qe, qs)))
        out.append((qt, recs))
    return out


def make_text(rng, n_contigs, n_max, L, style, shaped, prefix="c"):
    """shaped: the share of the records whose tag is shaped (random_tag)."""
    rows = []
    for c, (qt, recs) in enumerate(intervals(rng, n_contigs, n_max, L, style)):
        for qs, qe in recs:
            if style == 1 and rows and rng.random() < 0.15 and rows[-1].startswith("%s%d\t" % (prefix, c)):
                rows.append(rows[-1])                                # an exact duplicate row
                continue
            tag, rl, mat, aln = random_tag(rng, qe - qs + 1, rng.random() < shaped)
            rs = rng.randrange(0, 100000)
            rows.append("\t".join(["%s%d" % (prefix, c), str(qt), str(qs), str(qe + 1), rng.choice("+-"), rng.choice(REFS), "250000", str(rs), str(rs + rl),
                                   str(mat), str(aln), str(rng.choice((0, 0, 10, 60))), "tp:A:P", tag]))
    return ("\n".join(rows) + "\n").encode()


@functools.lru_cache(maxsize=None)
def shaped_text(i):
    """Shaped text number i: six contigs of 1 - 25 records, L = 400, style i % 3."""
    return make_text(random.Random("%d shaped %d" % (SEED, i)), 6, 25, 400, STYLES[i % 3], 1.0)


@functools.lru_cache(maxsize=None)
def unshaped_text(i):
    return make_text(random.Random("%d unshaped %d" % (SEED, i)), 6, 25, 400, STYLES[i % 3], SHAPED_SHARE)


@functools.lru_cache(maxsize=1)
def many_contigs_text(seed, style):
    """2 700 contigs of at most 14 records, L = 300, shaped tags (above 2 560 contigs the sweeps run two contigs per wave)."""
    return make_text(random.Random("%d many %d %d" % (SEED, seed, style)), 2700, 14, 300, style, 1.0)


def joined(texts):
    """Several texts as one file: contig names made distinct by the text's number."""
    return b"".join(b"".join(b"t%d_" % k + ln + b"\n" for ln in t.split(b"\n") if ln) for k, t in enumerate(texts))


Expected = collections.namedtuple("Expected", "kind files message sol verdict st")
ERR_FLAG = {"Alignment was clipped inside a cs insertion": 0x20, "Edited cs tag does not match edited PAF coordinates": 0x40}


@functools.lru_cache(maxsize=8)                                      # (a test's routes ask for the same run a few times in a row)
def _expected(T, text, K, nsl):
    io = T.io_oracle()
    st = io.read_paf(text)
    sol = T.oracle_solve(T.io_oracle_batch(st), K, nsl)
    verdict = {}
    cmain = [c for c in range(sol["n_contigs"]) for _ in range(int(sol["main_off"][c]), int(sol["main_off"][c + 1]))]
    calt = [c for c in range(sol["n_contigs"]) for _ in range(int(sol["alt_off"][c]), int(sol["alt_off"][c + 1]))]
    call = [c for c in range(sol["n_contigs"]) for p in range(int(sol["all_path_off"][c]), int(sol["all_path_off"][c + 1]))
            for _ in range(int(sol["all_elem_off"][p]), int(sol["all_elem_off"][p + 1]))]
    for k, ctg in (("main", cmain), ("alt", calt), ("all", call)):
        v = []
        for c, e in zip(ctg, sol[k]):
            try:
                io.get_edited_paf_data(int(e["qs"]), int(e["qe"]), int(e["rs"]), int(e["re"]), st.paf_data[c][int(e["ctg_index"])])
                v.append(0)
            except io.CsLogicError as err:
                v.append(ERR_FLAG[str(err)])
        verdict[k] = v
    try:
        return Expected("ok", io.render_outputs(st, sol), None, sol, verdict, st)
    except io.CsLogicError as err:
        return Expected("err", None, str(err), sol, verdict, st)


def expected(T, text, K, nsl):
    """The oracle side alone: I/O oracle reader -> solver oracle -> I/O oracle writers.  -> Expected: kind "ok" with the three files
    as bytes, or "err" with the message the reference would throw; the oracle's solution; verdict[list][i]: 0, or the cut-plan
    error flag of the exception get_edited_paf_data raises on that element."""
    return _expected(T, text, int(K), bool(nsl))
