"""A deterministic corpus of text inputs for the native readers of user-supplied text -- spl_bed_open and spl_gff_open
(csrc/spl_host.cpp) and the .SpliSER.tsv parser of csrc/spl_combine.cpp -- for test_text_fuzz.py (the readers against the Python
they stand in for) and test_native_sanitizers.py (the same code in an ASan + UBSan build).  No tests in here.

Three kinds of file per format, all as bytes:

* ``generated``: 2 to 6 seed lines (taken from the goldens and from the odd lines of test_text_native.py / test_combine_native.py),
  a share of them with one to three byte-level edits (insert, delete, replace) from ``ALPHABET`` under a fixed seed, and now and
  then a file-level edit on top (truncation at an arbitrary byte, no final newline, CRLF throughout, a blank last line);
* ``file_level``: the file-level edits once each on an unharmed file, with the empty file and the header-only table, and all of
  them once more filled up in front so that the file ends where its last page ends (the readers map their files);
* ``STRUCTURED``: one case per sentence of the parsers' contract, the accepted form next to its refused neighbour, each with the
  side it must land on ("accept": the native reader takes it and says what Python says; "refuse": SPL_ERR_FORMAT, the caller
  reads the file in Python).

Also here, because both suites and the sanitizer driver (tests/native/text_asan_driver.cpp) need one statement of them: the
checksum of a parsed file (``checksum``, CRC-32, over one text line per row), the value lists of the two number-format tests, the corner
CIGARs of the host packer's test and the small tables the driver runs the writers and the gene search on."""
import os
import random
import zlib

import numpy as np

SEED = 20240917
N_GENERATED = 3000
# share of a file's lines that get edits: tuned until every format has at least a fifth of its files on either side
# (test_text_fuzz.py asserts the shares; a .SpliSER.tsv line has hardly a byte its parser does not read)
MUTATION_RATE = {"bed": 0.55, "gff": 0.6, "tsv": 0.3}
FILE_EDIT_RATE = 0.08

# what the edits insert: separators of every parser here, the characters of Python's number grammar, control bytes that Python's
# str.strip / int() take for blanks (0x1c-0x1f among them) or that end a C string, line ends, and bytes outside ASCII
ALPHABET = [b"\t", b" ", b",", b";", b"=", b'"', b":", b"{", b"}", b"[", b"]",
            b"+", b"-", b"_", b".", b"e",
            b"7", b"07", b"1234567890123456789",
            b"\x00", b"\x0b", b"\x0c", b"\x1c", b"\x1f", b"\x7f",
            b"\r", b"\n",
            "é".encode("utf-8"), b"\xff"]

BED_SEEDS = [
    b"track name=junctions\n",
    b"Chr1\t705\t1763\tJUNC\t38\t+\t705\t1763\t255,0,0\t2\t10,10\t0,1048\n",
    b"Chr1\t705\t1216\tJUNC\t4\t-\t705\t1216\t255,0,0\t2\t10,10\t0,501\n",
    b"c1\t100\t300\tJ1\t7\t+\t100\t300\t0\t2\t10,20\t0,180\n",
    b"c2\t 5 \t900\tJ2\t+3\t\t5\t900\t0\t2\t1,2,\t0,1\n",                      # blanks, sign, empty strand, trailing comma
    b"c1\t100\t300\tJ3\t1\t-\t100\t300\t0\t2\t10,20\n",                         # 11 columns: skipped
    b"c1\t100\t300\tJ4\t1\t-\t100\t300\t0\t2\t10,20\t0,1\textra\n",             # 13 columns: skipped
    b"c1\t10\t3000000000\tJ5\t0\t?\t1\t2\t0\t2\t0,0\t0,1\n",
    b"scaffold_9\t0\t12\tJ6\t-0\t.\t0\t12\t0\t2\t007,0\t0,1\n",
]

GFF_SEEDS = [
    b"##gff-version 3\n",
    b"\n",
    b"   \n",
    b"Chr1\tsynth\tgene\t500\t3230\t.\t+\t.\tID=GChr1_0\n",
    b"Chr1\tsynth\tgene\t4290\t7743\t.\t-\t.\tID=GChr1_1;Name=x\n",
    b"c1\tsrc\tgene\t51\t320\t.\t+\t.\tID=G1;Name=x\n",
    b"c1\tsrc\tmRNA\t51\t320\t.\t+\t.\tID=G1.1\n",
    b'c2\tsrc\tgene\t5000\t6000\t.\t-\t.\t gene_id "G 2" ; other "y"\n',        # GTF style, quotes
    b"c1\tsrc\tgene\t10\t20\t.\t.\t.\tG3\n",                                    # bare name, strand '.'
    b"c1\tsrc\tgene\t10\t20\t.\t+\n",                                           # 7 columns: skipped
    b"c1\tsrc\tgene\t51\t99\t.\t-\t.\tID=G4\n",                                 # same left as G1: after it
    b"c2\tsrc\tgene\t 7 \t+9\t.\t+\t.\tID=G5\textra\n",                         # blanks and a sign in int(), a tenth column
]

TSV_HEADER = (b"Region\tSite\tStrand\tGene\tSSE\talpha_count\tbeta1_count\tbeta2Simple_count\tbeta2Cryptic_count\tbeta2Cryptic_weighted\t"
              b"Partners\tCompetitors\n")
TSV_SEEDS = [
    b"Chr1\t715\t+\tGChr1_0\t0.894\t42\t2\t3\tNA\tNA\t{1753: 38, 1206: 4, 1203: 0}\t[]\n",
    b"Chr1\t1203\t+\tGChr1_0\t0.000\t0\t0\t46\tNA\tNA\t{715: 0}\t[1206, 1753]\n",
    b"Chr1\t1206\t-\tNA\t0.080\t4\t2\t44\tNA\tNA\t{715: 4}\t[1203, 1753]\n",
    b"Chr1\t1753\t+\tGChr1_0\t0.905\t38\t0\t3\t1\t1.00000\t{715: 38}\t[1203, 1206]\n",
    b"Chr1\t1915\t?\tGChr1_1\t0.000\t0\t1\t4\t0\t0.00000\t{2196: 0}\t[]\n",
    b"Chr2\t100\t+\tNA\t0.500\t4\t2\t2\tNA\tNA\t{200: 4}\t[300]\n",
    b"Chr2\t2438\t-\tG2\t1.000\t1\t0\t0\t12\t2.33333\t{}\t[2984]\n",
    b"scaffold_9\t77\t+\tGChr1_0\t0.333\t1\t2\t0\t3\t1.5e-05\t{2438: 1}\t[]\n",
]
# the unharmed sample every .SpliSER.tsv of the corpus is combined with (test_combine_native.py: _compare on [good, mutated])
TSV_GOOD = TSV_HEADER + b"".join([
    b"Chr1\t715\t+\tGChr1_0\t0.885\t54\t4\t3\tNA\tNA\t{1753: 46, 1206: 8, 1203: 0}\t[1405]\n",
    b"Chr1\t1206\t+\tGChr1_0\t0.129\t8\t2\t52\tNA\tNA\t{715: 8}\t[1203, 1753]\n",
    b"Chr1\t1915\t+\tGChr1_1\t0.000\t0\t3\t2\t2\t0.50000\t{2196: 0}\t[]\n",
    b"Chr2\t100\t-\tNA\t0.250\t1\t2\t1\tNA\tNA\t{200: 1, 250: 0}\t[300, 310]\n",
    b"scaffold_9\t77\t+\tGChr1_0\t0.000\t0\t12\t0\tNA\tNA\t{}\t[]\n",
])
QUERY_GENE = b"GChr1_0"                 # the gene of the -g runs

SEEDS = {"bed": BED_SEEDS, "gff": GFF_SEEDS, "tsv": TSV_SEEDS}
EXT = {"bed": ".bed", "gff": ".gff", "tsv": ".SpliSER.tsv"}


def _edit(rng, line):
    n = rng.randint(1, 3)
    for _ in range(n):
        op = rng.choice(("insert", "delete", "replace"))
        at = rng.randrange(len(line) + 1) if op == "insert" else (rng.randrange(len(line)) if line else 0)
        tok = rng.choice(ALPHABET)
        if op == "insert" or not line:
            line = line[:at] + tok + line[at:]
        elif op == "delete":
            line = line[:at] + line[at + 1:]
        else:
            line = line[:at] + tok + line[at + 1:]
    return line


def truncated(data, rng):
    return data[:rng.randrange(len(data) + 1)]


def no_final_newline(data):
    return data[:-1] if data.endswith(b"\n") else data


def crlf(data):
    return data.replace(b"\n", b"\r\n")


def blank_last_line(data):
    return data + b"\n"


def _file_edit(rng, data):
    k = rng.randrange(4)
    return (truncated(data, rng), no_final_newline(data), crlf(data), blank_last_line(data))[k]


def generated(fmt, n=N_GENERATED):
    """-> [(name, bytes)]: n files of 2 to 6 seed lines, the same ones on every call."""
    rng = random.Random("%d-%s" % (SEED, fmt))
    out = []
    for k in range(n):
        lines = [rng.choice(SEEDS[fmt]) for _ in range(rng.randint(1 if fmt == "tsv" else 2, 5 if fmt == "tsv" else 6))]
        if fmt == "tsv":
            lines.sort(key=lambda l: (SEEDS[fmt].index(l)))      # (region by region, as `process` writes them)
            lines.insert(0, TSV_HEADER)
        lines = [_edit(rng, l) if rng.random() < MUTATION_RATE[fmt] else l for l in lines]
        data = b"".join(lines)
        if rng.random() < FILE_EDIT_RATE:
            data = _file_edit(rng, data)
        out.append(("g%04d" % k, data))
    return out


def _whole(fmt):
    return (TSV_HEADER if fmt == "tsv" else b"") + b"".join(SEEDS[fmt][:6] if fmt != "tsv" else SEEDS[fmt])


def file_level(fmt):
    """-> [(name, bytes, side)]: every file-level edit on an unharmed file; side None where the cut decides it."""
    whole = _whole(fmt)
    rng = random.Random("%d-%s-cuts" % (SEED, fmt))
    out = [("whole", whole, "accept"), ("empty", b"", "accept"), ("no_final_newline", no_final_newline(whole), "accept"),
           # (a blank line is no row of a .SpliSER.tsv: Python's _parse_tsv raises IndexError on it)
           ("blank_last_line", blank_last_line(whole), "refuse" if fmt == "tsv" else "accept"),
           # (the table parser refuses every carriage return; the two line readers take "\r\n" as text mode does)
           ("crlf", crlf(whole), "refuse" if fmt == "tsv" else "accept")]
    if fmt == "tsv":
        out.append(("header_only", TSV_HEADER, "accept"))
        out.append(("header_without_newline", TSV_HEADER[:-1], "accept"))
    for k in range(24):
        out.append(("cut%02d" % k, truncated(whole, rng), None))
    # The readers map their file: a read a few bytes past its end stays inside the last page, where no sanitizer sees it.  So
    # every file above once more, filled up IN FRONT (a line no reader reads) to end exactly where its last page ends: the byte
    # after it belongs to no page of the file.
    out += [("page_" + name, _to_page_end(fmt, data), side) for name, data, side in out if data]
    return out


PAGE = 4096


def _to_page_end(fmt, data):
    room = -len(data) % PAGE
    if fmt == "tsv":                       # (the first line is the header, whatever it says)
        return b"x" * room + data
    if room == 0:
        return data
    return (b"#" if fmt == "gff" else b"x") * (room - 1) + b"\n" + data


# ---- structured cases -----------------------------------------------------------------------------------------------------
def _bed(chrom=b"c1", start=b"100", stop=b"300", score=b"7", strand=b"+", sizes=b"10,20", tail=b"\t0,180", end=b"\n"):
    return b"\t".join([chrom, start, stop, b"J", score, strand, b"100", b"300", b"0", b"2", sizes]) + tail + end


def _gff(chrom=b"c1", kind=b"gene", c4=b"51", c5=b"320", strand=b"+", attr=b"ID=G1", more=b"", end=b"\n"):
    return b"\t".join([chrom, b"src", kind, c4, c5, b".", strand, b".", attr]) + more + end


def _tsv(chrom=b"Chr2", pos=b"100", strand=b"+", gene=b"NA", sse=b"0.500", alpha=b"4", beta1=b"2", b2s=b"2", b2c=b"NA", b2w=b"NA",
         partners=b"{200: 4}", competitors=b"[300]", end=b"\n"):
    return TSV_HEADER + b"\t".join([chrom, pos, strand, gene, sse, alpha, beta1, b2s, b2c, b2w, partners, competitors]) + end


D18, D19 = b"123456789012345678", b"1234567890123456789"
ARABIC_THREE = "٣".encode("utf-8")

STRUCTURED = {
    "bed": [
        # -- py_int: Python's int() for what occurs in these files: blanks, one sign, up to 18 decimal digits
        ("int_blanks", _bed(start=b" 5 "), "accept"),
        ("int_plus", _bed(score=b"+3"), "accept"),
        ("int_underscore", _bed(start=b"1_0"), "refuse"),                 # int("1_0") is 10
        ("int_18_digits", _bed(stop=D18), "accept"),
        ("int_19_digits", _bed(stop=D19), "refuse"),                      # Python has no limit; the reader's is 18 digits
        ("int_minus_zero", _bed(score=b"-0"), "accept"),
        ("int_leading_zeros", _bed(start=b"007"), "accept"),
        ("int_empty", _bed(start=b""), "refuse"),                         # Python: ValueError
        ("int_arabic_digit", _bed(start=ARABIC_THREE), "refuse"),         # int("٣") is 3
        ("int_float", _bed(score=b"7.0"), "refuse"),                      # Python: ValueError
        ("int_sign_then_blank", _bed(score=b"+ 3"), "refuse"),            # Python: ValueError
        ("int_blank_0x1f", _bed(start=b"\x1f5"), "refuse"),               # a blank to str.strip(), none to int(): ValueError
        ("int_blank_0x0b", _bed(start=b"5\x0b"), "accept"),
        ("int_0x7f", _bed(start=b"5\x7f"), "refuse"),                     # no blank: Python: ValueError
        # -- columns
        ("columns_11", _bed(tail=b""), "accept"),                         # skipped by both
        ("columns_12", _bed(), "accept"),
        ("columns_13", _bed(tail=b"\t0,180\textra"), "accept"),           # skipped by both
        ("columns_11_bad_number", _bed(start=b"x", tail=b""), "accept"),  # ... unread
        # -- block sizes
        ("sizes_two", _bed(sizes=b"10,20"), "accept"),
        ("sizes_trailing_comma", _bed(sizes=b"1,2,"), "accept"),
        ("sizes_three", _bed(sizes=b"1,2,x"), "accept"),                  # the third is never read
        ("sizes_one", _bed(sizes=b"10"), "refuse"),                       # Python: IndexError
        ("sizes_one_and_comma", _bed(sizes=b"10,"), "refuse"),            # Python: ValueError on ""
        # -- strand column
        ("strand_0_bytes", _bed(strand=b""), "accept"),
        ("strand_1_byte", _bed(strand=b"?"), "accept"),
        ("strand_2_bytes", _bed(strand=b"+-"), "refuse"),                 # the column is a byte here
        ("strand_control_byte", _bed(strand=b"\x0b"), "accept"),
        ("strand_nul", _bed(strand=b"\x00"), "refuse"),                   # came back as "no strand" where Python has "\x00"
        ("strand_two_byte_character", _bed(strand="é".encode("utf-8")), "refuse"),
        # -- bytes a C string or an ASCII reader cannot carry
        ("chrom_plain", _bed(chrom=b"c 2"), "accept"),
        ("chrom_nul", _bed(chrom=b"c\x002"), "refuse"),                   # came back as "c" where Python keeps "c\x002"
        ("nul_in_unread_column", _bed(tail=b"\t0,\x00180"), "refuse"),    # the whole file is refused, as the table parser does
        ("nul_in_skipped_line", b"track\x00\n" + _bed(), "refuse"),
        ("lone_0xff", _bed(tail=b"\t0,\xff180"), "refuse"),               # Python: UnicodeDecodeError
        ("two_byte_character_in_name", _bed(chrom="Chré".encode("utf-8")), "refuse"),
        ("del_in_name", _bed(chrom=b"c\x7f2"), "accept"),
        # -- line ends
        ("crlf", _bed(end=b"\r\n"), "accept"),
        ("lone_carriage_return", _bed(end=b"\rc2\n"), "refuse"),          # ends a line in Python
        ("carriage_return_at_end_of_file", _bed(end=b"\r"), "accept"),
        ("no_newline", _bed(end=b""), "accept"),
    ],
    "gff": [
        ("columns_8", _gff()[:_gff().rindex(b"\t")] + b"\n", "accept"),  # skipped by both
        ("columns_9", _gff(), "accept"),
        ("columns_10", _gff(more=b"\tmore;x=y"), "accept"),               # the ninth column ends at the tab
        ("type_gene", _gff(kind=b"gene"), "accept"),
        ("type_genes", _gff(kind=b"genes", c4=b"x"), "accept"),           # not a gene line: unread
        ("type_Gene", _gff(kind=b"Gene", c4=b"x"), "accept"),
        ("comment", b"#c1\tsrc\tgene\tx\n" + _gff(), "accept"),
        ("blank_lines", b"\n \t \n\x1f\n" + _gff(), "accept"),
        ("strand_dot", _gff(strand=b"."), "accept"),
        ("strand_empty", _gff(strand=b""), "refuse"),                     # Python keeps ""; the column is a byte here
        ("strand_2_bytes", _gff(strand=b"+-"), "refuse"),
        ("coordinate_blanks_sign", _gff(c4=b" 7 ", c5=b"+9"), "accept"),
        ("coordinate_underscore", _gff(c5=b"3_20"), "refuse"),
        ("coordinate_18_digits", _gff(c5=D18), "accept"),
        ("coordinate_19_digits", _gff(c5=D19), "refuse"),
        ("coordinate_empty", _gff(c4=b""), "refuse"),                     # Python: ValueError
        ("coordinate_blank_0x0c", _gff(c4=b"51\x0c"), "accept"),
        ("coordinate_blank_0x1c", _gff(c4=b"51\x1c"), "refuse"),          # a blank to str.strip(), none to int(): ValueError
        # -- the name: value of the first attribute
        ("attr_id", _gff(attr=b"ID=x"), "accept"),
        ("attr_gtf", _gff(attr=b'gene_id "x"'), "accept"),
        ("attr_gtf_more", _gff(attr=b' gene_id "G 2" ; other "y"'), "accept"),
        ("attr_bare", _gff(attr=b"x"), "accept"),
        ("attr_no_key", _gff(attr=b"=x"), "accept"),
        ("attr_blank_in_key", _gff(attr=b"a b=c"), "accept"),
        ("attr_quoted_pair", _gff(attr=b'"a=b"'), "accept"),
        ("attr_quotes_inside", _gff(attr=b'gene_id "x"y"z"'), "accept"),
        ("attr_only_quotes", _gff(attr=b'ID=""""'), "accept"),
        ("attr_empty", _gff(attr=b""), "accept"),
        ("attr_semicolon_first", _gff(attr=b";ID=x"), "accept"),
        ("attr_value_then_0x1f", _gff(attr=b"ID=7G3\x1f"), "accept"),     # str.strip() takes 0x1c-0x1f: named "7G3\x1f" once
        ("attr_0x1c_before_value", _gff(attr=b"ID=\x1c7G3;x=y"), "accept"),
        ("attr_0x1e_around_pair", _gff(attr=b"\x1eID=7G3\x1d;x"), "accept"),
        ("attr_value_then_0x0c", _gff(attr=b"ID=7G3\x0c"), "accept"),
        ("attr_0x1f_inside_value", _gff(attr=b"ID=7\x1fG3"), "accept"),   # kept by both
        ("attr_value_then_0x7f", _gff(attr=b"ID=7G3\x7f"), "accept"),     # no blank: kept by both
        ("attr_nul", _gff(attr=b"ID=7G3\x00"), "refuse"),
        ("attr_two_byte_character", _gff(attr="ID=géne".encode("utf-8")), "refuse"),
        ("chrom_nul", _gff(chrom=b"c\x002"), "refuse"),
        ("nul_in_comment", b"#\x00\n" + _gff(), "refuse"),
        ("lone_0xff_in_unread_line", _gff(kind=b"mRNA", attr=b"ID=\xff") + _gff(), "refuse"),   # Python: UnicodeDecodeError
        ("crlf", _gff(end=b"\r\n"), "accept"),
        ("lone_carriage_return", _gff(attr=b"ID=a\rb"), "refuse"),
        ("no_newline", _gff(end=b""), "accept"),
    ],
    "tsv": [
        # -- plain_int: [-]digits and nothing else, as `process` writes them
        ("int_plain", _tsv(pos=b"100"), "accept"),
        ("int_negative", _tsv(alpha=b"-4"), "accept"),
        ("int_blanks", _tsv(pos=b" 5 "), "refuse"),                       # int(" 5 ") is 5: Python's to read
        ("int_plus", _tsv(alpha=b"+3"), "refuse"),
        ("int_underscore", _tsv(pos=b"1_0"), "refuse"),
        ("int_18_digits", _tsv(b2s=D18), "accept"),
        ("int_19_digits", _tsv(b2s=D19), "refuse"),
        ("int_three_times_18_digits", _tsv(alpha=b"9" * 18, beta1=b"9" * 18, b2s=b"9" * 18), "accept"),   # the sums stay below 2^63
        ("int_minus_zero", _tsv(beta1=b"-0"), "accept"),
        ("int_empty", _tsv(beta1=b""), "refuse"),
        ("int_arabic_digit", _tsv(pos=ARABIC_THREE), "refuse"),
        ("int_float", _tsv(pos=b"100.0"), "refuse"),
        # -- plain_float: [-]digits[.digits][e[+-]digits], at most 47 characters
        ("float_dot_after", _tsv(sse=b"1."), "accept"),
        ("float_dot_before", _tsv(sse=b".5"), "accept"),
        ("float_exponent", _tsv(sse=b"1e5"), "accept"),
        ("float_exponent_sign", _tsv(b2c=b"3", b2w=b"1.5E-05"), "accept"),
        ("float_minus_only", _tsv(sse=b"-"), "refuse"),
        ("float_dot_only", _tsv(sse=b"."), "refuse"),
        ("float_inf", _tsv(sse=b"inf"), "refuse"),                        # float("inf") is a number
        ("float_nan", _tsv(sse=b"nan"), "refuse"),
        ("float_underscore", _tsv(sse=b"1_0.5"), "refuse"),               # float("1_0.5") is 10.5
        ("float_47_characters", _tsv(sse=b"0." + b"3" * 45), "accept"),
        ("float_48_characters", _tsv(sse=b"0." + b"3" * 46), "refuse"),
        ("float_empty_exponent", _tsv(sse=b"1e"), "refuse"),
        # -- cryptic columns
        ("cryptic_na", _tsv(b2c=b"NA", b2w=b"anything"), "accept"),       # the weighted column is not read then
        ("cryptic_numbers", _tsv(b2c=b"12", b2w=b"2.33333"), "accept"),
        ("cryptic_na_weighted_only", _tsv(b2c=b"12", b2w=b"NA"), "refuse"),
        # -- Partners {int: int, ...} and Competitors [int, ...]
        ("dict_empty", _tsv(partners=b"{}"), "accept"),
        ("dict_blank_inside", _tsv(partners=b"{ }"), "accept"),
        ("dict_spaced", _tsv(partners=b"{ 1 : 2 }"), "accept"),
        ("dict_tight", _tsv(partners=b"{1:2}"), "accept"),
        ("dict_leading_zeros", _tsv(partners=b"{007: 1}"), "refuse"),     # a SyntaxError to literal_eval
        ("dict_minus_zero", _tsv(partners=b"{-0: 1}"), "accept"),
        ("dict_trailing_comma", _tsv(partners=b"{1: 2,}"), "refuse"),     # fine to Python: Python's to read
        ("dict_duplicate_key", _tsv(partners=b"{200: 4, 200: 5}"), "refuse"),
        ("dict_blank_before", _tsv(partners=b" {1: 2}"), "refuse"),       # literal_eval strips it
        ("dict_no_value", _tsv(partners=b"{1}"), "refuse"),
        ("dict_unclosed", _tsv(partners=b"{1: 2"), "refuse"),
        ("list_empty", _tsv(competitors=b"[]"), "accept"),
        ("list_blank_inside", _tsv(competitors=b"[ ]"), "accept"),
        ("list_two", _tsv(competitors=b"[1 , 2]"), "accept"),
        ("list_double_comma", _tsv(competitors=b"[1,,2]"), "refuse"),
        ("list_trailing_comma", _tsv(competitors=b"[300,]"), "refuse"),
        ("list_tuple", _tsv(competitors=b"(300,)"), "refuse"),
        ("list_leading_zero", _tsv(competitors=b"[01]"), "refuse"),
        # -- lines
        ("columns_11", b"h\nChr1\t100\t+\n", "refuse"),                   # Python: IndexError
        ("columns_13", _tsv(end=b"\tmore\n"), "accept"),
        ("trailing_blanks", _tsv(end=b" \t \n"), "accept"),               # line.rstrip()
        ("trailing_0x1f", _tsv(end=b"\x1f\n"), "refuse"),                 # rstrip() takes it: Python's to read
        ("header_anything", b"\x7f whatever\n" + _tsv()[len(TSV_HEADER):], "accept"),
        ("crlf", crlf(_tsv()), "refuse"),
        ("nul", _tsv(gene=b"G\x00"), "refuse"),
        ("two_byte_character", _tsv(gene="géne".encode("utf-8")), "refuse"),
        ("lone_0xff", _tsv(gene=b"\xff"), "refuse"),
        ("no_newline", _tsv(end=b""), "accept"),
    ],
}


def corpus(fmt):
    """-> [(name, bytes, side or None)] of one format: the generated files, the file-level edits, the structured cases."""
    return ([(n, d, None) for n, d in generated(fmt)] + [("f_" + n, d, s) for n, d, s in file_level(fmt)] +
            [("s_" + n, d, s) for n, d, s in STRUCTURED[fmt]])


def write_corpus(root):
    """The corpus as files under root/<format>/.  -> {format: [(name, path, side or None)]}; root/good.SpliSER.tsv is TSV_GOOD."""
    out = {}
    with open(os.path.join(root, "good.SpliSER.tsv"), "wb") as fh:
        fh.write(TSV_GOOD)
    for fmt in ("bed", "gff", "tsv"):
        os.makedirs(os.path.join(root, fmt), exist_ok=True)
        out[fmt] = []
        for name, data, side in corpus(fmt):
            path = os.path.join(root, fmt, name + EXT[fmt])
            with open(path, "wb") as fh:
                fh.write(data)
            out[fmt].append((name, path, side))
    return out


# ---- the checksum of a parsed file: the driver prints it, test_native_sanitizers.py computes it through the ordinary library ------
checksum = zlib.crc32       # chained over the pieces of a job: checksum(piece, checksum_so_far)


def columns_text(cols, with_names):
    """One line per row of a native.TextColumns: chromosome name, left, right, then alpha and the strand byte (BED) or the strand
    byte and the gene's name (GFF)."""
    rows = []
    for i in range(cols.chrom.shape[0]):
        head = "%s\t%d\t%d\t" % (cols.chrom_names[int(cols.chrom[i])], int(cols.left[i]), int(cols.right[i]))
        rows.append(head + ("%d\t%s\n" % (int(cols.strand[i]), cols.names[i]) if with_names else "%d\t%d\n" % (int(cols.alpha[i]), int(cols.strand[i]))))
    return "".join(rows).encode("latin-1")


# the runs of `combine` the driver makes on every table it accepts: (gene, shallow or None, cryptic and stranded)
COMBINE_RUNS = [(g, s, c) for g in ("All", QUERY_GENE.decode()) for s in (None, (1, 2, 0.1)) for c in (False, True)]


def first_appearance(runs):
    seen = []
    for mine in runs:
        for chrom in mine:
            if chrom not in seen:
                seen.append(chrom)
    return seen


# ---- number formats: the value lists of test_tsv_native.py and test_combine_native.py ---------------------------------------------
def fixed_values():
    """Ratios of small integers (exact ties like 1/16 included), random doubles, powers of two, tiny and large values: all >= 0."""
    rnd = random.Random(7)
    values = [0.0, 1.0, 0.5, 0.0625, 0.1875, 0.0005, 0.00049999999999999, 0.9995, 0.99949999999999994, 2.5e-5, 5e-324, 1e-310,
              123456789.123456, 8.9e12, 4503599627370496.0, 1e40, 0.000005, 0.0000049999]
    values += [2.0 ** -k for k in range(0, 80)] + [(2 * k + 1) / 2.0 ** 12 for k in range(0, 2048, 7)]
    values += [a / b for a in range(0, 60) for b in range(1, 60)]
    values += [rnd.random() for _ in range(20000)] + [rnd.random() * 10 ** rnd.randint(-8, 12) for _ in range(20000)]
    values += [rnd.randint(0, 10 ** 6) / 10 ** rnd.randint(1, 7) for _ in range(20000)]   # decimal-looking values next to ties
    return values


def repr_values():
    rng = np.random.default_rng(7)
    vals = [0.0, -0.0, 2.0, 0.33333, 12.5, 1e16, 1e15, 9999999999999998.0, 1.5e-5, 1e-4, 9.999e-5, 1e22, 5e-324, 1.7976931348623157e308,
            0.1 + 0.2, 100.0, 123456.789, float("inf"), float("-inf")]
    vals += (rng.integers(0, 10 ** 7, 3000) / 1e5).tolist()                      # what "{0:.5f}" of process leaves, summed or not
    vals += (rng.integers(0, 10 ** 7, 500) / 1e5 + rng.integers(0, 10 ** 7, 500) / 1e5).tolist()
    vals += np.exp(rng.uniform(-60, 60, 3000)).tolist()
    vals += rng.standard_normal(500).tolist()
    return vals


FIXED_DIGITS = (3, 5, 0, 6)

# ---- the host packer: the corner CIGARs of test_pack_host.py ----------------------------------------------------------------------
PACK_CORNER_RECORDS = [
    (0, 100, "50M"), (16, 100, "50="), (0, 100, "20M100N30M"), (0, 100, "5S20M100N30M3S"), (0, 100, "20M100N30M50N40M"),
    (0, 100, "2H20M2I100N30M50N40M1P"), (4, 100, "50M"), (0, 100, "*"), (0, 100, "10S"), (0, 100, "10M5D10M"),
    (0, 100, "10M0N10M"), (0, 100, "10M5N5N10M"), (0, 100, "10N20M"), (0, 100, "20M10N"), (0, 100, "70000M"),
    (0, 100, "70000M10N5M"), (0, 100, "5M10N70000M"), (0, 100, "5M10N5M10N70000M"), (0, 100, "1M1N1M1N1M1N1M"),
    (0, 100, "1M1I1M1I1M1I1M1I1M"), (0, 100, "1M1D" * 10), (1024, 2147483000, "1000M"), (0, 2147483000, "100M")]

# ---- the gene search on the tables its bisection is awkward on: (left, right, strands) and the positions asked ---------------------
GENE_TABLES = [
    ("empty", [], [], b""),
    ("one_gene", [10], [20], b"+"),
    ("equal_left", [10, 10, 10, 30], [20, 40, 15, 50], b"+-+-"),
]
GENE_QUERY_POS = list(range(0, 60, 5))
GENE_QUERY_STRANDS = b"+-?"

# ---- the two writers on small arrays: 0 rows, an empty name ----------------------------------------------------------------------
# (what the driver hands spl_tsv_append_many: a chromosome "" of two rows, one of no rows, "c2" of one row with one partner position
#  on two edges; and the text it must leave, without and with the cryptic columns)
APPEND_MANY_TEXT = {
    False: (b"\t100\t+\tG\t0.500\t4\t2\t2\tNA\tNA\t{200: 4}\t[300]\n"
            b"\t150\t\t\t0.000\t0\t0\t0\tNA\tNA\t{}\t[]\n"
            b"c2\t7\t-\tNA\t1.000\t1\t0\t0\tNA\tNA\t{9: 1}\t[8, 9]\n"),
    True: (b"\t100\t+\tG\t0.500\t4\t2\t2\t1\t0.50000\t{200: 4}\t[300]\n"
           b"\t150\t\t\t0.000\t0\t0\t0\t0\t0.00000\t{}\t[]\n"
           b"c2\t7\t-\tNA\t1.000\t1\t0\t0\t3\t1.66667\t{9: 1}\t[8, 9]\n"),
}
BEDGRAPH_RUNS = [("", [0, 5], [5, 9], [3, 0], 0), ("c1", [], [], [], 0), ("c1", [10, 20, 30], [20, 30, 31], [1, 4000000000, 7], 3)]
