"""Random PAF texts for the device reader's differential tests (tests/test_read_fuzz_cpu.py, tests/test_gpu_read_fuzz.py): valid
texts that vary everything the reader frames (structured), byte edits of them (mutate), and an independent count of the rows whose
numbers are off the device's fast path (expected_slow).  Nothing here comes from the product; everything follows from the
random.Random it is given."""
import functools
import random
import re

from read_cases import GOOD, TAGS, TILE, consumed

EDGE_OFFSETS = (0, 1, 7, 8, 15, 16, 17)
NEAR_MISSES = [b"cs:Z", b"xcs:Z::5", b"cs:z::7", b"acs:Z::3:3", b"CS:Z::4", b"cs:Z"]
OTHER_TAGS = [b"tp:A:P", b"NM:i:12", b"ms:i:4071", b"AS:i:-3", b"de:f:0.0012", b"zd:i:1", b"rl:i:0", b"zz:Z:" + b"x" * 40, b"cg:Z:10M2I3D", b""]
ALPHABET = [b"\t", b"\n", b"\r", b"\r\n", b"-", b"+", b"0", b"9", b":", b" ", b"c", b"cs:Z:", b"x", b"", b"1234567890123456789"]
NUMERIC_COLUMNS = (1, 2, 3, 6, 7, 8, 9, 10, 11)
FAST_NUMBER = re.compile(rb"-?[0-9]{1,18}")
NAME_BYTES = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_.|:-"


def random_cs(rng, target):
    """A valid short-form cs string of about `target` bytes."""
    ops, n = [], 0
    while n < target:
        k = rng.random()
        if k < 0.4:
            op = b":%d" % rng.choice((1, 2, 9, 10, 123, rng.randrange(1, 100000)))
            if rng.random() < 0.05:
                op = b":" + b"0" * rng.randrange(1, 20) + op[1:]
        elif k < 0.6:
            op = b"*" + bytes(rng.choice(b"acgtn") for _ in range(2))
        else:
            m = rng.choice((1, 2, 5, 40, min(max(1, target - n), rng.randrange(1, 3000))))
            op = rng.choice((b"+", b"-")) + bytes(rng.choice(b"acgtACGT") for _ in range(min(m, 64))) * (m // 64 + 1)
            op = op[:m + 1]
        ops.append(op)
        n += len(op)
    return b"".join(ops)


def _name(rng, lo=0):
    n = rng.choice((lo, 1, 4, 4, 5, 8, 8, 12, 40, rng.randrange(lo, 301)))
    return bytes(rng.choice(NAME_BYTES) for _ in range(max(n, lo)))


def _number(rng, v, zeros):
    """v as the text of a PAF column; zeros: leading zeros up to 18 digits in all."""
    s = b"%d" % abs(v)
    if zeros and len(s) < 18 and rng.random() < 0.15:
        s = b"0" * rng.randrange(1, 19 - len(s)) + s
    return (b"-" if v < 0 or (v == 0 and zeros and rng.random() < 0.02) else b"") + s


def _wide(rng, signed):
    """A number of 1 - 18 digits."""
    v = rng.randrange(10 ** rng.randrange(0, 18), 10 ** 18) if rng.random() < 0.2 else rng.randrange(0, 10 ** rng.randrange(1, 10))
    return -v if signed and rng.random() < 0.1 else v


def _row(rng, name, ref, cs, strict, eol, pad=None):
    """One valid row; strict: inside what the I/O oracle models (see read_cases.py); pad: the row's length in bytes."""
    ql, rl = consumed(cs)
    qs = rng.choice((0, 7, 100, rng.randrange(0, 10 ** 9), _wide(rng, True) // 10))
    rs = rng.choice((0, 1000, rng.randrange(0, 10 ** 9), _wide(rng, True) // 10))
    mat, aln, mq = rng.randrange(0, 1 << 31), rng.randrange(0, 1 << 31), rng.randrange(0, 256)
    if not strict and rng.random() < 0.1:
        mat, aln, mq = _wide(rng, True), _wide(rng, True), rng.randrange(-300, 1000)       # truncated to 32 / 8 bits
    cols = [name, _number(rng, _wide(rng, True), True), _number(rng, qs, True), _number(rng, qs + ql, True), rng.choice((b"+", b"-")), ref,
            _number(rng, _wide(rng, True), True), _number(rng, rs, True), _number(rng, rs + rl, True), _number(rng, mat, True), _number(rng, aln, True), _number(rng, mq, True)]
    if not strict and rng.random() < 0.03:                           # off the fast path, and still a number to strtoll
        k = rng.choice((1, 6, 9, 10))
        cols[k] = rng.choice((b"+" + cols[k].lstrip(b"-"), b" " + cols[k], b"1" + b"0" * 18, b"9" * 25, b"0" * 19 + cols[k].lstrip(b"-")))
    before = [rng.choice(OTHER_TAGS[:-1] + NEAR_MISSES) for _ in range(rng.choice((0, 1, 1, 2, rng.randrange(0, 13))))]
    after = [rng.choice(OTHER_TAGS + NEAR_MISSES + [b"cs:Z::99"]) for _ in range(rng.choice((0, 0, 1, rng.randrange(0, 13))))]
    if len(before) + len(after) > 12:
        after = after[:12 - len(before)]
    r = b"\t".join(cols + before + [b"cs:Z:" + cs] + after) + eol
    if pad is not None:
        if len(r) + 6 > pad:                                         # too long to pad: a short row of the same names instead
            r = b"\t".join(cols[:12] + [b"cs:Z:" + cs]) + eol
        if len(r) + 6 > pad:
            return None
        r = r[:-len(eol)] + b"\tzz:Z:" + b"x" * (pad - len(r) - 6) + eol
    return r


def structured(rng):
    """A valid text -> (text, strict).  strict: LF line ends and nothing of what the I/O oracle does not model, so its arrays can
    be compared as well."""
    strict = rng.random() < 0.4
    eol = b"\n" if strict or rng.random() < 0.5 else b"\r\n"
    refs = list({_name(rng) for _ in range(rng.choice((1, 2, 4, 4, 8, rng.randrange(1, 121))))})
    n_rows = rng.choice((1, 2, 5, 20, 60, 150, rng.randrange(1, 400)))
    budget = rng.choice((1, 1, 1, 2, 2, 3, 5)) * TILE                # about this many bytes
    rows, size, ref, names = [], 0, rng.choice(refs), set()

    def pad_to_edge():
        """The next row ends near a tile edge: the one after it, or the text's end, is at k * TILE + d."""
        nonlocal size
        d = rng.choice(EDGE_OFFSETS) * rng.choice((-1, 1))
        k = (size + 300) // TILE + 1
        r = _row(rng, name, ref, GOOD, strict, eol, pad=k * TILE + d - size)
        if r is not None:
            rows.append(r)
            size += len(r)

    while len(rows) < n_rows and size < budget:
        name = _name(rng, 1 if strict else 0)
        if name in names:
            continue
        names.add(name)
        for _ in range(rng.choice((1, 1, 2, 3, 5, rng.randrange(1, 13)))):
            if rng.random() < 0.5:
                ref = rng.choice(refs)                               # (else the row before's: runs, and names that come back)
            k = rng.random()
            cs = rng.choice(TAGS) if k < 0.7 else random_cs(rng, rng.choice((5, 20, 100, 300, 1000, rng.randrange(5, 20001))))
            r = _row(rng, name, ref, cs, strict, eol)
            rows.append(r)
            size += len(r)
            if rng.random() < 0.03:
                pad_to_edge()
            if rng.random() < 0.05:
                blank = eol if strict else rng.choice((eol, b"\r\n", b"\n", b"\n\n\r\n"))   # (a lone '\r' is a row to the oracle)
                rows.append(blank)
                size += len(blank)
    if rng.random() < 0.7:
        pad_to_edge()
    text = b"".join(rows)
    if rng.random() < 0.4:
        text = text[:-len(eol)]                                      # no final newline
    return text, strict


def mutate(rng, text):
    """1 - 4 edits of the text: insert, replace or delete at a random offset, half of them within 20 bytes of a tile edge or of
    the text's end."""
    t = bytearray(text)
    for _ in range(rng.randrange(1, 5)):
        if rng.random() < 0.5:
            edges = [k * TILE for k in range(1, len(t) // TILE + 1)] + [len(t)]
            at = rng.choice(edges) + rng.randrange(-20, 21)
        else:
            at = rng.randrange(0, len(t) + 1)
        at = min(max(at, 0), len(t))
        what, tok = rng.randrange(3), rng.choice(ALPHABET)
        if what == 0:
            t[at:at] = tok
        elif what == 1:
            t[at:at + max(1, len(tok))] = tok
        else:
            del t[at:at + rng.randrange(1, 6)]
    return bytes(t)


def lines(text):
    """(start, line) of the text's rows: split at '\\n', one trailing '\\r' dropped, empty lines skipped."""
    out, p = [], 0
    for ln in text.split(b"\n"):
        body = ln[:-1] if ln.endswith(b"\r") else ln
        if body:
            out.append((p, body))
        p += len(ln) + 1
    return out


def expected_slow(text):
    """Rows with twelve or more columns one of whose nine numbers is not [-] and 1 - 18 digits.  (Means something only for a text
    the host reader takes: there each of them is a number to strtoll.)"""
    n = 0
    for _, ln in lines(text):
        f = ln.split(b"\t")
        if len(f) >= 12 and not all(FAST_NUMBER.fullmatch(f[k]) for k in NUMERIC_COLUMNS):
            n += 1
    return n


def row_start_near_edge(text):
    """Does a row start within 16 bytes of a tile edge (not the text's start)?"""
    return any(p >= TILE - 16 and min(p % TILE, TILE - p % TILE) <= 16 for p, _ in lines(text))


# ---- the corpora of both tiers: text number i of a kind follows from (SEED, kind, i) alone
SEED = 20261017


@functools.lru_cache(maxsize=8)
def structured_text(i):
    """Structured text number i -> (text, strict)."""
    return structured(random.Random("%d structured %d" % (SEED, i)))


def mutant_text(i):
    """Mutant number i: edits of structured text number i // 3."""
    return mutate(random.Random("%d mutant %d" % (SEED, i)), structured_text(i // 3)[0])
