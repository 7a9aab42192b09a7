"""Hand-made alt texts for the --alt merge on the device (tests/test_alt_device_cpu.py, tests/test_gpu_alt_device.py,
tests/test_cli_alt_device.py): every rule of merge_alt_text once, over a small synthetic main file, and the texts the device
declines.  Each case says what it is meant to do as a check on the HOST route's result (meant(main, merged)), which
alt_testlib.host_route runs on the CPU before the case is used.

An alt row is a row of the main file (so its tag fits its coordinates) under a piece name, with columns 2 (qry_total) and 11
(aln_len) set to give the ratio the case needs."""
import os

import numpy as np

GOLDEN_FILES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "files")
DEVICE_SAYS = "aasm_paf_merge_alt_device: the device does not merge this alt text (%s, alt row %d); merge on the host"
WHY_ZEROED = "a group without a positive ratio"
WHY_PIECE_NUMBER = "a piece start that is not 1 - 18 digits"


def main_text(api, n_contigs=4, recs=8, seed=21):
    return api.Paf.synth(n_contigs, recs, seed).to_text()


def contig_names(text):
    names = []
    for line in text.decode().splitlines():
        q = line.split("\t")[0]
        if not names or names[-1] != q:
            names.append(q)
    return names


def alt_row(src, piece, aln, qtot, ref=None, strand=None, extra_tags=None, **cols):
    """Line `src` of a main file under the piece name `piece` with aln_len / qry_total = aln / qtot; cols: {column index: text}."""
    f = src.split("\t")
    f[0], f[1], f[10] = piece, str(qtot), str(aln)
    if ref is not None:
        f[5] = ref
    if strand is not None:
        f[4] = strand
    if extra_tags:
        cs = next(i for i in range(12, len(f)) if f[i].startswith("cs:Z:"))
        f[cs:cs] = list(extra_tags)
    for k, v in cols.items():
        f[int(k[1:])] = v
    return "\t".join(f)


def _text(rows, end="\n", final=True):
    return (end.join(rows) + (end if final else "")).encode()


def _added(main, merged):
    """Per contig: the rows a merge appended, as (row_index, qry_total, ref_chr)."""
    mo, go = main["view"]["ctg_rec_off"], merged["view"]["ctg_rec_off"]
    out = []
    for c in range(len(mo) - 1):
        lo, hi = int(go[c] + (mo[c + 1] - mo[c])), int(go[c + 1])
        assert np.all(merged["cols"]["cord_type"][lo:hi] == 1) and np.all(merged["cols"]["cord_type"][int(go[c]):lo] == 0)
        out.append([(int(merged["cols"]["row_index"][g]), int(merged["view"]["qry_total"][g]), int(merged["view"]["ref_chr"][g])) for g in range(lo, hi)])
    return out


def _rows_of(main, merged):
    return [[r for r, _, _ in ctg] for ctg in _added(main, merged)]


def merging_cases(api):
    """[{name, main, alt, baseline, meant, oracle}]: texts the device merges.  oracle: False where the I/O oracle cannot read the
    text (it splits lines at line feeds only, and counts ':' by parsing the tag)."""
    cases = []
    tiny, tiny_alt = (open(os.path.join(GOLDEN_FILES, n), "rb").read() for n in ("tiny.paf", "tiny_alt.paf"))
    for b in (0.0, 0.5, 0.9, 1.0):
        cases.append(dict(name=f"tiny_{b}", main=tiny, alt=tiny_alt, baseline=b, meant=lambda m, g: sum(map(len, _added(m, g))) > 0, oracle=True))
    main = main_text(api)
    L = main.decode().splitlines()
    N = contig_names(main)
    assert len(N) == 4 and len(L) == 32

    def add(name, rows, meant, baseline=0.5, main=main, oracle=True, **kw):
        cases.append(dict(name=name, main=main, alt=rows if isinstance(rows, bytes) else _text(rows, **kw), baseline=baseline, meant=meant, oracle=oracle))

    p = lambda c, start, span=5000: f"{N[c]}:{start}-{start + span - 1}"
    # group A: two rows over, one under: exactly the two; group B: none over: the first row of its largest ratio
    add("over_and_under", [alt_row(L[0], p(0, 101), 800, 1000), alt_row(L[1], p(0, 101), 200, 1000), alt_row(L[2], p(0, 101), 900, 1000),
                           alt_row(L[3], p(0, 7001), 100, 1000), alt_row(L[4], p(0, 7001), 300, 1000), alt_row(L[5], p(0, 7001), 200, 1000)],
        lambda m, g: _rows_of(m, g) == [[0, 2, 4], [], [], []])
    # a ratio equal to the baseline is not "over": were it, both 0.5 rows would be kept; as the best row, only the first is
    add("equal_to_baseline", [alt_row(L[8], p(1, 11), 500, 1000), alt_row(L[9], p(1, 11), 500, 1000), alt_row(L[10], p(1, 11), 250, 1000)],
        lambda m, g: _rows_of(m, g) == [[], [0], [], []])
    add("tie_first_wins", [alt_row(L[8], p(1, 11), 200, 1000), alt_row(L[9], p(1, 11), 400, 1000), alt_row(L[10], p(1, 11), 400, 1000), alt_row(L[11], p(1, 11), 100, 1000)],
        lambda m, g: _rows_of(m, g) == [[], [1], [], []])
    add("unknown_contig_goes_to_0", [alt_row(L[16], "nosuch_ctg:11-900", 900, 1000), alt_row(L[17], p(2, 11), 900, 1000)],
        lambda m, g: _rows_of(m, g) == [[0], [], [1], []])
    # one contig name heads two separate runs of the main file: the piece resolves to the last
    twice = _text(L[0:8] + L[8:16] + [ln.replace(N[2], N[0], 1) for ln in L[16:24]] + L[24:32])
    assert contig_names(twice) == [N[0], N[1], N[0], N[3]]
    add("repeated_name_resolves_to_last", [alt_row(L[0], p(0, 101), 900, 1000), alt_row(L[24], p(3, 101), 900, 1000)],
        lambda m, g: _rows_of(m, g) == [[], [], [0], [1]], main=twice)
    # pieces of contig 0 that are not adjacent in the alt file: three runs of contig 0 interleaved with contig 1's
    add("interleaved_runs", [alt_row(L[0], p(0, 101), 900, 1000), alt_row(L[1], p(0, 101), 700, 1000), alt_row(L[8], p(1, 101), 900, 1000),
                             alt_row(L[2], p(0, 20001), 600, 1000), alt_row(L[9], p(1, 20001), 100, 1000), alt_row(L[10], p(1, 20001), 800, 1000),
                             alt_row(L[3], p(0, 40001), 300, 1000), alt_row(L[4], p(0, 40001), 200, 1000)],
        lambda m, g: _rows_of(m, g) == [[0, 1, 3, 6], [2, 5], [], []])
    # a contig whose main records differ in qry_total: its LAST record's is inherited
    odd = L[:]
    f = odd[7].split("\t"); f[1] = str(int(f[1]) + 12345); odd[7] = "\t".join(f)
    last_qtot = int(f[1])
    add("last_records_qry_total", [alt_row(L[0], p(0, 101), 900, 777)], lambda m, g: _added(m, g)[0] == [(0, last_qtot, _added(m, g)[0][0][2])] and last_qtot != int(L[0].split("\t")[1]),
        main=_text(odd))
    # reference names: new in a dropped row and used again in a kept row; numbered over ALL rows by first appearance
    n_chr = lambda m: int(m["cols"]["n_chr"])
    add("new_reference_names", [alt_row(L[0], p(0, 101), 100, 1000, ref="chrNewB"), alt_row(L[1], p(0, 101), 900, 1000, ref="chrNewA_longer_than_eight"),
                                alt_row(L[2], p(0, 9001), 900, 1000, ref="chrNewB"), alt_row(L[3], p(0, 9001), 100, 1000, ref="chrNewC")],
        lambda m, g: n_chr(g) == n_chr(m) + 3 and [r[2] for r in _added(m, g)[0]] == [n_chr(m) + 1, n_chr(m)]
        and g["cols"]["names"].tobytes().endswith(b"chrNewBchrNewA_longer_than_eightchrNewC"))
    add("known_reference_names", [alt_row(L[0], p(0, 101), 900, 1000, ref=L[31].split("\t")[5]), alt_row(L[9], p(1, 101), 900, 1000)],
        lambda m, g: n_chr(g) == n_chr(m) and sum(map(len, _added(m, g))) == 2)
    add("minus_strand", [alt_row(L[0], p(0, 101), 900, 1000, strand="-"), alt_row(L[1], p(0, 101), 800, 1000, strand="+")],
        lambda m, g: _rows_of(m, g)[0] == [0, 1] and [int(x) for x in g["view"]["aln_fwd"][int(g["view"]["ctg_rec_off"][1]) - 2:int(g["view"]["ctg_rec_off"][1])]] == [0, 1])
    # CRLF line ends, blank lines between rows, no final line feed: row_index counts non-empty lines
    rows = [alt_row(L[0], p(0, 101), 100, 1000), "", alt_row(L[1], p(0, 101), 900, 1000), "", "", alt_row(L[8], p(1, 5), 900, 1000)]
    add("crlf_blank_lines_no_final_lf", rows, lambda m, g: _rows_of(m, g) == [[1], [2], [], []], end="\r\n", final=False, oracle=False)
    add("tags_before_cs", [alt_row(L[0], p(0, 101), 900, 1000, extra_tags=("NM:i:12", "cs:i:5", "zz:Z:cs:Z::9"))], lambda m, g: _rows_of(m, g)[0] == [0])
    add("piece_name_without_dash", [alt_row(L[0], f"{N[0]}:123", 900, 1000), alt_row(L[1], f"{N[0]}:123", 950, 1000), alt_row(L[2], f"{N[0]}:123-", 950, 1000)],
        lambda m, g: _rows_of(m, g)[0] == [0, 1, 2] and int(g["view"]["qry_str"][int(g["view"]["ctg_rec_off"][1]) - 1]) == int(L[2].split("\t")[2]) + 122)
    # numbers off the reader's fast path that strtoll takes: the host resolves the row, the ratio included
    add("slow_numbers", [alt_row(L[0], p(0, 101), "+900", 1000), alt_row(L[1], p(0, 101), 100, " 1000"), alt_row(L[2], p(0, 101), 800, "+1000")],
        lambda m, g: _rows_of(m, g)[0] == [0, 2])
    # column 11 beyond 32 bits: the ratio is made of the full value (0.5000000006), the stored aln_len of its low half
    add("aln_len_beyond_32_bits", [alt_row(L[0], p(0, 101), 2 ** 32 + 5, 2 ** 33), alt_row(L[1], p(0, 101), 1, 2 ** 33)],
        lambda m, g: _rows_of(m, g)[0] == [0] and int(g["cols"]["aln_len"][int(g["view"]["ctg_rec_off"][1]) - 1]) == 5)
    add("no_rows_empty", b"", lambda m, g: sum(map(len, _added(m, g))) == 0 and g["view"]["n_records"] == m["view"]["n_records"], oracle=False)
    add("no_rows_blank_lines", b"\n\r\n\n", lambda m, g: sum(map(len, _added(m, g))) == 0, oracle=False)
    return cases


def declined_cases(api):
    """[{name, main, alt, baseline, says}]: texts the device declines.  says: None where the host route names the fault (its code
    and message are the entry's), else the device's own message for a text the host merges."""
    main = main_text(api)
    L = main.decode().splitlines()
    N = contig_names(main)
    p = lambda c, start, span=5000: f"{N[c]}:{start}-{start + span - 1}"
    good = [alt_row(L[0], p(0, 101), 900, 1000), alt_row(L[1], p(0, 101), 100, 1000)]
    cut = lambda line, n: "\t".join(line.split("\t")[:n])
    no_cs = lambda line: "\t".join(x for x in line.split("\t") if not x.startswith("cs:Z:"))
    cases = [
        dict(name="zeroed_group", alt=good + [alt_row(L[2], p(0, 9001), 0, 1000), alt_row(L[3], p(0, 9001), 0, 1000)], says=DEVICE_SAYS % (WHY_ZEROED, 2)),
        dict(name="nan_ratio_group", alt=[alt_row(L[2], p(0, 9001), 0, 0)] + good, says=DEVICE_SAYS % (WHY_ZEROED, 0)),
        dict(name="name_without_colon", alt=good + [alt_row(L[2], N[0], 900, 1000)], says=None),
        dict(name="name_x_9", alt=good + [alt_row(L[2], f"{N[0]}:x-9", 900, 1000)], says=None),
        dict(name="start_with_a_sign", alt=good + [alt_row(L[2], f"{N[0]}:+7-9", 900, 1000)], says=DEVICE_SAYS % (WHY_PIECE_NUMBER, 2)),
        dict(name="eleven_columns", alt=good + [cut(alt_row(L[2], p(0, 9001), 900, 1000), 11)], says=None),
        dict(name="no_cs_tag", alt=good + [no_cs(alt_row(L[2], p(0, 9001), 900, 1000))], says=None),
        dict(name="non_numeric_column", alt=good + [alt_row(L[2], p(0, 9001), 900, 1000, c7="12x")], says=None),
        dict(name="two_faults_first_is_named", alt=[good[0], alt_row(L[2], p(0, 9001), 900, 1000, c8="n/a"), good[1], alt_row(L[3], N[0], 900, 1000)], says=None),
        dict(name="two_faults_other_order", alt=[good[0], alt_row(L[3], N[0], 900, 1000), good[1], cut(alt_row(L[2], p(0, 9001), 900, 1000), 9)], says=None),
    ]
    for c in cases:
        c.update(main=main, alt=_text(c["alt"]), baseline=0.5)
    return cases


def bad_tag_case(api):
    """A well-formed alt row whose tag is malformed: the device merges it, the merged batch's solve reports it."""
    main = main_text(api)
    L = main.decode().splitlines()
    N = contig_names(main)
    row = alt_row(L[0], f"{N[0]}:101-5100", 900, 1000)
    f = row.split("\t")
    cs = next(i for i in range(12, len(f)) if f[i].startswith("cs:Z:"))
    f[cs] = f[cs][:9] + "!" + f[cs][9:]
    return dict(name="bad_tag", main=main, alt=_text(["\t".join(f)]), baseline=0.5)


def big_case(api, n_contigs=40, recs=30, seed=5):
    """At least 1 100 alt rows in more than two reader tiles: every main row as an alt row, in groups of one to four rows on pieces
    of several contigs (some unknown), ratios on both sides of the baseline, reference names known and new; no zeroed group."""
    main = main_text(api, n_contigs, recs, seed)
    L = main.decode().splitlines()
    N = contig_names(main)
    rows, i, g = [], 0, 0
    while i < len(L):
        n = 1 + (g * 7 + 3) % 4
        c = (g * 13) % (len(N) + 3)
        name = N[c] if c < len(N) else f"unknown{c}"
        piece = f"{name}:{1 + 1000 * (g % 50)}-{999999}"
        for t in range(min(n, len(L) - i)):
            aln = 1 + ((i * 37 + t * 211) % 1000)
            ref = None if i % 5 else f"alt_ref_{(i // 5) % 23}"
            rows.append(alt_row(L[i], piece, aln, 1000, ref=ref))
            i += 1
        g += 1
    alt = _text(rows)
    assert len(rows) >= 1100 and len(alt) > 2 * 16384
    return dict(name="big", main=main, alt=alt, baseline=0.5, meant=lambda m, g: 100 < sum(map(len, _added(m, g))) < len(rows), oracle=True)
