"""Texts for the device reader's tests (tests/test_read_cpu.py, tests/test_gpu_read.py): what aasm_paf_parse_device must read as
the host reader does.  A case is {name, text, oracle, slow, weak}:
  oracle  the independent reader (oracle/paf_io_oracle.py) models this text, so its arrays are compared too.  It splits lines on
          '\\n' alone, takes numbers with Python's int() and keeps them unbounded, and checks every tag against the coordinates;
          where a case needs what it does not model, the case's comment says so and the host reader alone is the yardstick.
  slow    rows whose numbers are off the device's fast path ([-] and 1 - 18 digits): exactly these the host may patch.
  weak    run again with AASM_READ_H_WEAK_HASH (reference names collide all the time).
few_blocks(case): run again on the device with AASM_READ_H_FEW_BLOCKS (the emulation caps its grids for every case).
Nothing here depends on the product: the texts are built from bytes."""
import re

TILE = 16384                      # AASM_READ_TILE (asserted by the CPU tier)
GOOD = b":10*ac:5+gg:3-t:2"

# the tag list of tests/test_cs_device.py
TAGS = [
    b":10*ac:5+gg:3-t:2", b":1", b"*ag", b"+" + b"acgt" * 40 + b":7", b":5-" + b"t" * 150 + b":9*ct:123456", b":" + b"9" * 7 + b"+a",
    (b":12*ac" * 30) + b":4", b":3" + b"+a:1" * 70, b":007*ac:00000000000000000000005+GG:0012",
]


def consumed(cs):
    q = r = 0
    for op in re.findall(rb":[0-9]+|\*[A-Za-z][A-Za-z]|[+-][A-Za-z]+", cs):
        if op[:1] == b":": q += int(op[1:]); r += int(op[1:])
        elif op[:1] == b"*": q += 1; r += 1
        elif op[:1] == b"+": q += len(op) - 1
        else: r += len(op) - 1
    return q, r


def row(name=b"ctg1", cs=GOOD, fwd=True, qs=100, ref=b"chr1", rs=1000, tags=None, eol=b"\n", **over):
    """One PAF row whose coordinates fit the tag.  tags: the whole tag list (default tp + the cs tag); over: raw bytes for the
    columns qtot, qs, qe, strand, rtot, rs, re, mat, aln, mq."""
    ql, rl = consumed(cs)
    f = {"qtot": b"100000", "qs": b"%d" % qs, "qe": b"%d" % (qs + ql), "strand": b"+" if fwd else b"-", "rtot": b"5000000",
         "rs": b"%d" % rs, "re": b"%d" % (rs + rl), "mat": b"10", "aln": b"10", "mq": b"60"}
    f.update(over)
    if tags is None:
        tags = [b"tp:A:P", b"cs:Z:" + cs]
    return b"\t".join([name, f["qtot"], f["qs"], f["qe"], f["strand"], ref, f["rtot"], f["rs"], f["re"], f["mat"], f["aln"], f["mq"]] + list(tags)) + eol


def fill(n, seed=0, eol=b"\n", name=None):
    """Valid rows of exactly n bytes together (n >= 200), contigs of three rows, four reference names, both strands."""
    out, left, i = [], n, seed
    while left > 0:
        nm = name or b"ctg%d" % (i // 3)
        r = row(nm, TAGS[i % 3], fwd=bool(i % 2), qs=100 + 50 * (i % 90), ref=b"chr%d" % (i % 4), eol=eol)
        if left < len(r) + 120:                                      # the last row: padded by a tag behind the cs tag to fit
            base = row(nm, GOOD, qs=7, ref=b"chrL", tags=[b"tp:A:P", b"cs:Z:" + GOOD, b"zz:Z:"], eol=eol)
            assert left >= len(base), (n, left)
            r = row(nm, GOOD, qs=7, ref=b"chrL", tags=[b"tp:A:P", b"cs:Z:" + GOOD, b"zz:Z:" + b"x" * (left - len(base))], eol=eol)
        out.append(r)
        left -= len(r)
        i += 1
    text = b"".join(out)
    assert len(text) == n
    return text


def case(name, text, oracle=True, slow=0, weak=False):
    return {"name": name, "text": text, "oracle": oracle, "slow": slow, "weak": weak}


def long_tag(L):
    return b":5+" + b"a" * L + b":7"


# tags without a row start inside: a tile's worth less 200, a tile, a tile and a byte, three tiles and five, 1 MiB (64 tiles)
LONG = [("tile_minus_200", TILE - 200), ("tile", TILE), ("tile_plus_1", TILE + 1), ("three_tiles_plus_5", 3 * TILE + 5), ("1mib", 1 << 20)]
BIG = {"qtot": b"9000000"}                # (a query long enough for the long tags)


def slow_text(n_rows, every, bad=None):
    """n_rows rows, all different, row i off the fast path (three forms in turn) where i % every == 0; bad: the number of the slow
    row (from 1) whose rtot no reader takes."""
    rows, k = [], 0
    for i in range(n_rows):
        over = {}
        if i % every == 0:
            k += 1
            over = ({"rtot": b"+%d" % (5000000 + i)}, {"qtot": b" %d" % (100000 + i)}, {"rtot": b"1" + b"%018d" % i})[k % 3]
            if k == bad:
                over = {"rtot": b"5x"}
        rows.append(row(b"ctg%d" % (i // 7), TAGS[i % 3], fwd=bool(i % 2), qs=100 + 13 * i, ref=b"chr%d" % (i % 5), rs=1000 + 7 * i, **over))
    return b"".join(rows), k


def long_cases():
    """Rows of kilobytes to a megabyte: tiles without a row start, tags and names across tile edges."""
    c = []
    crlf = b"\r\n"
    for name, L in LONG:
        cs = long_tag(L)
        c.append(case("long_%s_only" % name, row(b"ctgL", cs, **BIG)))
        c.append(case("long_%s_between" % name, fill(1000) + row(b"ctgL", cs, fwd=False, **BIG) + fill(1000, 5)))
        c.append(case("long_%s_last_open" % name, fill(1000) + row(b"ctgL", cs, **BIG)[:-1]))
        c.append(case("long_%s_crlf" % name, fill(1000, eol=crlf) + row(b"ctgL", cs, eol=crlf, **BIG) + fill(700, 2, eol=crlf), oracle=False))   # (CR: see crlf_lines)
    cs = long_tag(3 * TILE + 5)
    c.append(case("long_second_cs_ignored", fill(700) + row(b"ctgL", tags=[b"tp:A:P", b"cs:Z:" + GOOD, b"cs:Z:" + long_tag(1 << 20)]) + fill(700, 4)))
    c.append(case("long_behind_long_other_tag", fill(700) + row(b"ctgL", cs, tags=[b"zz:Z:" + b"x" * (3 * TILE + 5), b"cs:Z:" + cs], **BIG) + row(b"ctgL", qs=300) + fill(700, 4)))
    c.append(case("long_70000_colons", row(b"ctgL", b":1*ac" * 70000, **BIG) + row(b"ctgL", qs=300000, **BIG) + row(b"ctgM", b":1*ac" * 70000, fwd=False, **BIG) + row(b"ctgM")))
    # ---- names
    q40, r40 = b"Q" * 39 + b"q", b"R" * 39 + b"r"
    a = row(q40) + row(q40, qs=300)                                  # the second row's query name lies on [TILE - 20, TILE + 20)
    b = row(b"ctgR", ref=r40) + row(b"ctgR", qs=300, ref=r40)        # the second row's reference name on [2 * TILE - 20, 2 * TILE + 20)
    head = fill(TILE - 20 - len(a) // 2) + a
    head += fill(2 * TILE - 20 - len(head) - len(b) // 2 - b.index(r40))
    c.append(case("names_straddle_tile_edges", head + b + row(b"ctgR", qs=500) + row(b"ctgR", qs=700, ref=r40) + fill(500, 3), weak=True))
    n5, r5 = b"n" * 4999, b"r" * 4999
    c.append(case("contig_names_5000_differ_in_last_byte", row(n5 + b"a") + row(n5 + b"a", qs=300) + row(n5 + b"b") + row(n5 + b"b", qs=300) + row(n5 + b"a", qs=500)))
    c.append(case("ref_names_5000_differ_in_last_byte", b"".join(row(b"ctg%d" % (i // 4), qs=100 + i, ref=r5 + (b"a", b"b", b"b", b"a", b"c")[i % 5]) for i in range(20)), weak=True))
    # an empty contig name: the oracle takes "" for "no contig yet" (alignasm.cpp:117) and merges such a contig with the next one
    c.append(case("empty_query_name", row(b"") + row(b"", qs=300) + row(b"ctg2") + row(b"", qs=500) + row(b"ctg2", qs=300), oracle=False))
    # ---- a row start in every tile, nothing else in it; then contigs of one row
    per_tile = []
    for i in range(20):
        base = row(b"tile%d" % (i // 2), GOOD, qs=100 + 40 * i, tags=[b"tp:A:P", b"cs:Z:" + GOOD, b"zz:Z:"])
        per_tile.append(row(b"tile%d" % (i // 2), GOOD, qs=100 + 40 * i, tags=[b"tp:A:P", b"cs:Z:" + GOOD, b"zz:Z:" + b"x" * (TILE - len(base))]))
    c.append(case("long_one_row_per_tile", b"".join(per_tile) + b"".join(row(b"c%d" % i, qs=100 + i, ref=b"chr%d" % (i % 3)) for i in range(200))))
    # ---- slow rows up to and beyond the bulk download of the row starts (read_run: n_slow > 64); see slow_numbers for the oracle
    for n_rows, every in ((640, 10), (650, 10), (600, 2)):
        text, k = slow_text(n_rows, every)
        c.append(case("slow_rows_%d" % k, text, oracle=False, slow=k))
    return c


def valid_cases(synth_text):
    """synth_text: a file of several hundred KB whose rows cross every kind of edge (Paf.synth(200, 50, ...).to_text())."""
    c = []
    one = row()
    # ---- line framing
    c.append(case("one_row", one))
    c.append(case("one_row_no_newline", one[:-1]))
    c.append(case("blank_lines", b"\n\n" + one + b"\n" + row(b"ctg2") + b"\n\n\n" + row(b"ctg2", qs=400) + b"\n"))
    # CR: the oracle splits on '\n' alone and would keep the '\r' in the last tag
    c.append(case("crlf_lines", fill(3000, eol=b"\r\n"), oracle=False))
    c.append(case("lone_cr_line", one + b"\r\n" + row(b"ctg2") + b"\r\n\r\n" + row(b"ctg3"), oracle=False))
    c.append(case("lone_cr_last_byte", one + row(b"ctg2") + b"\r", oracle=False))
    c.append(case("cr_then_eof_on_row", one + row(b"ctg2")[:-1] + b"\r", oracle=False))
    c.append(case("newline_last_byte_of_tile", fill(TILE) + fill(700, 5)))          # = a row start exactly on a tile edge
    c.append(case("newline_first_byte_of_tile", fill(TILE + 1) + fill(700, 5)))
    c.append(case("row_start_on_second_edge", fill(TILE - 300) + fill(TILE + 300, 7) + fill(900, 3)))
    c.append(case("crlf_split_by_tile_edge", fill(TILE + 1, eol=b"\r\n") + fill(600, 2, eol=b"\r\n"), oracle=False))   # '\r' the tile's last byte
    c.append(case("crlf_ends_tile", fill(TILE, eol=b"\r\n") + fill(600, 2), oracle=False))
    for extra in (1, 7, 8, 9, 15, 16, 17):
        c.append(case("len_tile_plus_%d" % extra, fill(TILE + extra)))
        c.append(case("len_tile_plus_%d_open" % extra, fill(TILE + extra + 1)[:-1]))                                  # no final newline
    c.append(case("synth_file", synth_text))
    # ---- tags
    c.append(case("cs_first", row(tags=[b"cs:Z:" + GOOD, b"tp:A:P"]) + row(b"ctg2", tags=[b"cs:Z:" + GOOD])))
    c.append(case("cs_behind_ten_tags", row(tags=[b"t%d:i:%d" % (i, i) for i in range(10)] + [b"cs:Z:" + GOOD]) + row(b"ctg2")))
    c.append(case("two_cs_tags", row(tags=[b"cs:Z:" + GOOD, b"cs:Z::99"]) + row(b"ctg2", tags=[b"tp:A:P", b"cs:Z:" + GOOD, b"cs:Z::1:1:1"])))
    c.append(case("near_tags", row(tags=[b"xcs:Z::5", b"cs:Z", b"cs:z::7", b"cs:Z:" + GOOD]) + row(b"ctg2", tags=[b"cs:Z", b"acs:Z::3:3", b"cs:Z:" + GOOD])))
    c.append(case("bare_cs", row(cs=b"") + row(b"ctg2", cs=b"", fwd=False) + row(b"ctg2", qs=300)))
    rows = []
    for k, cs in enumerate(TAGS):
        for fwd in (True, False):
            rows.append(row(b"ctg%d" % (k // 2), cs, fwd, qs=1000 * (len(rows) + 1)))
    c.append(case("cs_device_tag_list", b"".join(rows)))
    # ---- numbers
    c.append(case("negative_and_18_digits", row(rtot=b"-5") + row(qtot=b"1" + b"0" * 17, qs=300) + row(b"ctg2", rtot=b"-" + b"9" * 18)))
    # strtoll's leniency: the oracle's int() is another (it also takes "5 "), and it does not saturate
    c.append(case("slow_numbers", row(rtot=b"+5") + row(qtot=b" 5", qs=300) + row(b"ctg2", rtot=b"1" + b"0" * 18) + row(b"ctg2", qtot=b"9" * 25, qs=300) + row(b"ctg3"),
                  oracle=False, slow=4))
    c.append(case("slow_row_last_no_newline", row() + row(b"ctg2", rtot=b"+7")[:-1], oracle=False, slow=1))
    # the oracle keeps Python ints: no truncation to 32 / 8 bits
    c.append(case("truncating_columns", row(mat=b"%d" % ((1 << 32) + 7)) + row(aln=b"%d" % (1 << 31), qs=300) + row(b"ctg2", mq=b"300") + row(b"ctg2", mq=b"-1", qs=300), oracle=False))
    c.append(case("minus_strand", row(fwd=False) + row(fwd=False, qs=300) + row(b"ctg2")))
    # an empty strand column is '-' to the product (record_of); the oracle indexes its first character
    c.append(case("empty_strand", row(strand=b"") + row(b"ctg2", strand=b"+x") + row(b"ctg2", strand=b"*", qs=300), oracle=False))
    # ---- contigs
    c.append(case("ctg1_then_ctg10", row(b"ctg1") + row(b"ctg10") + row(b"ctg10", qs=300) + row(b"ctg1", qs=300) + row(b"ctg", qs=500)))
    c.append(case("name_comes_back", row(b"a") + row(b"b") + row(b"a", qs=300) + row(b"a", qs=500) + row(b"b", qs=300)))
    c.append(case("one_row_contigs", b"".join(row(b"c%d" % i, qs=100 + i) for i in range(150))))
    c.append(case("contig_spans_three_tiles", row(b"first") + fill(2 * TILE + 700, 3, name=b"wide") + row(b"last")))
    # ---- reference names, each again under the weak hash
    c.append(case("refs_reverse_alphabetical", b"".join(row(b"ctg%d" % (i // 4), qs=100 + i, ref=b"chr" + bytes([ord("z") - i % 7])) for i in range(40)), weak=True))
    c.append(case("refs_more_than_64", b"".join(row(b"ctg%d" % (i // 5), qs=100 + i, ref=b"ref_%d" % ((i * 37) % 90)) for i in range(400)), weak=True))
    c.append(case("refs_shared_prefix", b"".join(row(b"ctg%d" % (i // 3), qs=100 + i, ref=b"chromosome_%c%c" % (65 + i % 5, 65 + (i // 5) % 3)) for i in range(60)), weak=True))
    c.append(case("refs_runs_and_returns", b"".join(row(b"ctg%d" % (i // 6), qs=100 + i, ref=(b"chrB", b"chrB", b"chrA", b"chrB", b"", b"chrA")[i % 6]) for i in range(36)), weak=True))
    c += long_cases()
    names = [x["name"] for x in c]
    assert len(set(names)) == len(names)
    return c


def few_blocks(c):
    """Is the case read again with every grid capped at 3 blocks (AASM_READ_H_FEW_BLOCKS)?  Where that makes blocks take a second
    item: more than 3 tiles, more than 3 * 256 rows; and the cases named for it."""
    return (len(c["text"]) > 3 * TILE or c["text"].count(b"\n") > 768 or c["name"].startswith("long_")
            or c["name"] in ("synth_file", "refs_more_than_64"))


def error_cases():
    """(name, text): the reader's code and message are the host reader's - the first bad row in file order."""
    good = fill(1500)
    few = b"\t".join([b"ctgX", b"1000", b"1", b"2", b"+", b"chr1", b"9", b"1", b"2", b"3", b"4"]) + b"\n"      # 11 columns
    no_tag = row(b"ctgN", tags=[b"tp:A:P", b"xcs:Z::5", b"cs:Z"])
    twelve = row(b"ctgT", tags=[])
    bad_tag = row(b"ctgB", tags=[b"tp:A:P", b"cs:Z::10?:5"])
    e = [
        ("too_few_columns", good + few + good),
        ("no_cs_tag", good + no_tag + good),
        ("twelve_columns_no_tags", good + twelve),
        ("number_5x", good + row(b"ctgX", rtot=b"5x") + good),
        ("number_trailing_blank", good + row(b"ctgX", qtot=b"5 ") + good),
        ("number_empty_field", good + row(b"ctgX", mq=b"") + good),
        ("number_lone_minus", good + row(b"ctgX", mat=b"-") + good),
        ("later_kind_first", fill(TILE // 2) + no_tag + fill(2 * TILE, 3) + few + good),                            # two kinds, different tiles
        ("number_before_columns", fill(TILE // 2) + row(b"ctgX", aln=b"1e3") + fill(2 * TILE, 3) + few + good),
        ("columns_before_number", fill(TILE // 2) + few + fill(2 * TILE, 3) + row(b"ctgX", aln=b"1e3") + good),
        ("fault_in_last_row", good + few),
        ("fault_in_last_row_no_newline", good + no_tag[:-1]),
        ("bad_tag_before_column_fault", good + bad_tag + good + few + good),                                          # the earlier row's tag is the error
        ("slow_row_70_of_100_is_5x", slow_text(700, 7, bad=70)[0]),                                                   # behind 69 rows the host resolves
        ("empty_text", b""),
        ("only_blank_lines", b"\n\r\n\n"),
    ]
    return e


def bad_tag_only():
    """A file whose only defect is a malformed tag: reads fine, fails in the solve."""
    return fill(1500) + row(b"ctgB", tags=[b"tp:A:P", b"cs:Z::10?:5"]) + fill(900, 4)
