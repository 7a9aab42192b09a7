"""Texts for the tests of the device reader's resident row columns (tests/test_read_cols_cpu.py, tests/test_gpu_read_cols.py): the
smallest name shapes at which a lanes-per-name copy can go wrong.  The names kernel copies a name in 8-byte steps, sixteen lanes to
a name, and its last n % 8 bytes one by one: names of every length 1 .. 40 and around 64 and 128 stand beside one another, so a
byte dropped, doubled or written into the neighbour shows in `names`.  Cases have read_cases.case's shape; `few`: read again
with AASM_READ_H_FEW_BLOCKS on the device.  Nothing here depends on the product: the texts are built from bytes."""
import read_cases as RC

LENGTHS = list(range(1, 41)) + [63, 64, 65, 127, 128, 129]


def name_of(n, salt):
    """n bytes, every position its own letter (a shifted or repeated byte shows), different for every (n, salt)."""
    return bytes(97 + (5 * i + 3 * n + salt) % 26 for i in range(n))


def _case(name, text, few=False):
    c = RC.case(name, text, oracle=False)
    c["few"] = few
    return c


def name_cases():
    c = []
    # neighbouring contigs, a different name of every length; two rows each, one reference
    c.append(_case("contig_names_every_length", b"".join(RC.row(name_of(n, 0), qs=100) + RC.row(name_of(n, 0), qs=300) for n in LENGTHS)))
    # ... the same for the reference names: rows of three-row contigs, the name changing with every row, each length twice
    rows = [RC.row(b"ctg%d" % (i // 3), qs=100 + 40 * i, ref=name_of(n, 7)) for i, n in enumerate(LENGTHS + LENGTHS[::-1])]
    c.append(_case("ref_names_every_length", b"".join(rows)))
    c.append(_case("both_names_every_length", b"".join(RC.row(name_of(n, 1), qs=100, ref=name_of(m, 11)) for n, m in zip(LENGTHS, LENGTHS[::-1]))))
    c.append(_case("one_contig_one_ref", RC.row()))
    # every block of the names grid takes several names, under the capped grid many times over
    c.append(_case("one_row_contigs_2000", b"".join(RC.row(b"c%d" % i, qs=100 + i, ref=b"chr%d" % (i % 23)) for i in range(2000)), few=True))
    # the last row's names are new ones, and the row ends with the text: a bare tag and no newline are the shortest tail a row's
    # names can have behind them
    last = RC.row(name_of(65, 2), cs=b"", ref=name_of(129, 13), tags=[b"cs:Z:"])[:-1]
    c.append(_case("last_row_new_names_no_newline", RC.row() + RC.row(qs=300) + last))
    names = [x["name"] for x in c]
    assert len(set(names)) == len(names)
    return c


def case_ids():
    return [x["name"] for x in name_cases()]
