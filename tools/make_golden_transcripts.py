#!/usr/bin/env python3
"""Recipe of tests/golden/transcripts: runs the reference's countHitTranscripts.py (process() and the writer of its
main()) over small cases and records what it writes, or that it stops.  Never imported by a test.

    python tools/make_golden_transcripts.py [--reference /root/reference]

Per case: <case>/annotation.gff, <case>/crackling.csv and <case>/expected.csv (absent when the reference raises), and
cases.json with the list.  The cases over tests/golden/bowtie take the committed <config>.csv of that directory as their
Crackling file.  Every GFF is copied to a temporary directory first: the reference pickles what it loaded beside it.  The
inputs below are this project's own; nothing of the reference's text is copied but the sample of its useSampleData(), which
is data it reads."""
import argparse
import contextlib
import csv
import importlib.util
import io
import json
import pathlib
import shutil
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "tests" / "golden" / "transcripts"
BOWTIE = ROOT / "tests" / "golden" / "bowtie"
HEADER = "seq,bowtieChr,bowtieStart,bowtieEnd\n"


def gff(rows):
    """rows: (seq, type, start, end, attributes) -> GFF3 text."""
    return "".join(f"{s}\tcase\t{t}\t{a}\t{b}\t.\t+\t.\t{attr}\n" for s, t, a, b, attr in rows)


def queries(rows):
    return HEADER + "".join(f"G{n},{c},{s},{s + 22}\n" for n, (c, s) in enumerate(rows))


GENE = [
    ("c1", "gene", 1, 900, "ID=g1"),
    ("c1", "mRNA", 1, 900, "ID=t1;Parent=g1"),
    ("c1", "exon", 100, 200, "ID=e1;Parent=t1"),
    ("c1", "exon", 300, 400, "ID=e2;Parent=t1"),
    ("c1", "mRNA", 1, 900, "ID=t2;Parent=g1"),
    ("c1", "exon", 150, 250, "ID=e3;Parent=t2"),
]
PROBES = [("c1", s) for s in (99, 100, 149, 150, 200, 201, 250, 251, 300, 400, 401)]


def case_list(sample):
    cases = {}
    cases["sample"] = sample
    cases["dotted_names"] = (
        gff([("NC_1.4", "mRNA", 1, 900, "ID=t1;Parent=g1"), ("NC_1.4", "exon", 10, 50, "ID=e1;Parent=t1"),
             ("plain", "mRNA", 1, 900, "ID=t2;Parent=g2"), ("plain", "exon", 10, 50, "ID=e2;Parent=t2")]),
        queries([("NC_1.4", 20), ("NC_1_4", 20), ("plain", 20), ("pla.in", 20), ("NC_1_4", 51)]))
    cases["gene_lines"] = (
        gff([("c1", "gene", 1, 900, "ID=g1"), ("c2", "gene", 1, 900, "ID=g2;Parent=root"), ("c3", "gene", 1, 900, "Parent=root")]
            + GENE[1:]),
        queries(PROBES + [("c2", 5), ("c3", 5)]))
    cases["exon_without_mrna_first"] = (
        gff([("c1", "exon", 100, 200, "ID=e0;Parent=ghost")] + GENE),
        queries(PROBES))
    cases["exon_without_mrna_later"] = (
        gff([("c1", "mRNA", 1, 900, "ID=t1;Parent=g1"), ("c1", "exon", 100, 200, "ID=e1;Parent=t1"),
             ("c1", "exon", 150, 300, "ID=e0;Parent=ghost")]),
        queries([("c1", 120), ("c1", 160), ("c1", 250), ("c1", 301)]))
    cases["only_unmapped"] = (
        gff([("c1", "exon", 100, 200, "ID=e0;Parent=ghost"), ("c1", "exon", 150, 300, "ID=e1;Parent=spectre")]),
        queries([("c1", 120), ("c1", 160), ("c1", 99)]))
    cases["two_genes"] = (
        gff(GENE + [("c1", "mRNA", 1, 900, "ID=u1;Parent=g2"), ("c1", "exon", 180, 320, "ID=x1;Parent=u1")]),
        queries(PROBES + [("c1", 180), ("c1", 260), ("c1", 320)]))
    cases["duplicated_mrna"] = (
        gff(GENE + [("c1", "mRNA", 1, 900, "ID=t2;Parent=g1"), ("c1", "mRNA", 1, 900, "ID=t1;Parent=other")]),
        queries(PROBES))
    cases["id_on_two_sequences"] = (
        gff(GENE + [("c2", "exon", 100, 200, "ID=e9;Parent=t1"), ("c2", "mRNA", 1, 900, "ID=t2;Parent=g7"),
                    ("c2", "exon", 100, 120, "ID=e8;Parent=t2")]),
        queries(PROBES + [("c2", 100), ("c2", 121), ("c2", 201)]))
    cases["overlapping_exons"] = (
        gff(GENE + [("c1", "exon", 150, 350, "ID=e4;Parent=t1"), ("c1", "exon", 100, 200, "ID=e5;Parent=t1"),
                    ("c1", "exon", 100, 200, "ID=e6;Parent=t1")]),
        queries(PROBES + [("c1", 260)]))
    cases["adjacent_exons"] = (
        gff([("c1", "mRNA", 1, 900, "ID=t1;Parent=g1"), ("c1", "exon", 100, 199, "ID=e1;Parent=t1"),
             ("c1", "exon", 200, 300, "ID=e2;Parent=t1"), ("c1", "mRNA", 1, 900, "ID=t2;Parent=g1"),
             ("c1", "exon", 200, 200, "ID=e3;Parent=t2")]),
        queries([("c1", s) for s in (99, 100, 199, 200, 201, 300, 301)]))
    cases["start_above_end"] = (
        gff([("c1", "mRNA", 1, 900, "ID=t1;Parent=g1"), ("c1", "exon", 200, 100, "ID=e1;Parent=t1"),
             ("c1", "exon", 50, 60, "ID=e2;Parent=t1"), ("c1", "exon", 0, 3, "ID=e3;Parent=t1")]),
        queries([("c1", s) for s in (0, 3, 4, 50, 60, 100, 150, 200)]))
    crlf = gff(GENE).replace("\n", "\r\n")
    cases["crlf"] = (crlf, queries(PROBES).replace("\n", "\r\n"))
    cases["cr_only"] = (gff(GENE).replace("\n", "\r"), queries(PROBES).replace("\n", "\r"))
    cases["field_counts_and_comments"] = (
        "##gff-version 3\n# a comment\n\n" + gff(GENE)
        + "c1\tcase\tmRNA\t1\t900\t.\t+\tID=t8;Parent=g1\n"                         # 8 fields
        + "c1\tcase\tmRNA\t1\t900\t.\t+\t.\tID=t9;Parent=g1\textra\n"               # 10 fields
        + " c1 \tcase\t exon \t 120 \t 130 \t.\t+\t.\t ID=e7;Parent=t9 \n"          # stripped fields; t9 has no mRNA line
        + "c1\tcase\tCDS\t100\t200\t.\t+\t.\tID=c1;Parent=t1\n",
        queries(PROBES + [("c1", 125)]))
    cases["attribute_quirks"] = (
        gff([("c1", "mRNA", 1, 900, "ID=zz;ID=t1;Parent=g0;Parent=g1;Note=a=b"),
             ("c1", "exon", 100, 200, "ID=e1;Parent=t1=ignored;Name=x"),
             ("c1", "mRNA", 1, 900, "ID=t2;Parent=g1; Parent=g9"),
             ("c1", "exon", 150, 250, "ID=e2;Parent=t2;Parent =t7")]),
        queries([("c1", s) for s in (100, 150, 200, 250)]))
    cases["error_attribute_without_equals"] = (gff(GENE + [("c1", "exon", 1, 2, "ID=e9;Parent=t1;flag")]), queries(PROBES))
    cases["error_trailing_semicolon_other_type"] = (gff(GENE + [("c1", "CDS", 1, 2, "ID=c9;Parent=t1;")]), queries(PROBES))
    cases["error_empty_attributes"] = (gff(GENE) + "c1\tcase\tregion\t1\t2\t.\t+\t.\t\n", queries(PROBES))
    cases["error_exon_coordinate"] = (gff(GENE + [("c1", "exon", "12.5", 20, "ID=e9;Parent=t1")]), queries(PROBES))
    cases["error_exon_end"] = (gff(GENE + [("c1", "exon", 12, "", "ID=e9;Parent=t1")]), queries(PROBES))
    cases["bad_coordinate_on_mrna_is_fine"] = (gff(GENE + [("c1", "mRNA", "x", "y", "ID=t5;Parent=g1")]), queries(PROBES))
    cases["error_header_without_column"] = (gff(GENE), "seq,bowtieChr,bowtieStart\nG0,c1,100\n")
    cases["error_bowtie_start"] = (gff(GENE), HEADER + "G0,c1,100,122\nG1,c1,abc,122\n")
    cases["error_bowtie_end"] = (gff(GENE), HEADER + "G0,c1,100,1e3\n")
    cases["error_short_row"] = (gff(GENE), HEADER + "G0,c1,100,122\nG1,c1\n")
    cases["error_blank_row"] = (gff(GENE), HEADER + "G0,c1,100,122\n\nG1,c1,150,172\n")
    cases["csv_quoting"] = (
        gff(GENE),
        "note,seq,bowtieChr,bowtieStart,bowtieEnd,more\n"
        '"a,b",G0,c1,100,122,"say ""hi"""\n'
        '"two\nlines",G1,c1,150,172,\n'
        'plain,G2,"c1",201,223,"x"y\n'
        ',G3,?,?,?,"tail\r\nrow"\n'
        'q"uote,G4,*,0,22,a b\n'
        'last,G5,c1,300,322,"open\n')
    cases["error_single_empty_header"] = (gff(GENE), '""\n')
    cases["csv_empty_file"] = (gff(GENE), "")
    cases["csv_header_only"] = (gff(GENE), HEADER.rstrip("\n"))
    cases["star_and_question_rows"] = (
        gff(GENE + [("*", "mRNA", 1, 900, "ID=s1;Parent=gs"), ("*", "exon", 0, 10, "ID=se;Parent=s1"),
                    ("?", "mRNA", 1, 900, "ID=q1;Parent=gq"), ("?", "exon", 0, 10, "ID=qe;Parent=q1")]),
        HEADER + "G0,*,0,22\nG1,?,?,?\nG2,?,0,22\nG3,c1,100,122\nG4,*,11,33\nG5,?,abc,\n")
    cases["nothing_counted"] = (
        "##gff-version 3\n" + gff([("c1", "gene", 1, 900, "ID=g1"), ("c1", "region", 1, 900, "ID=r;Parent=x")]),
        queries(PROBES + [("*", 0)]))
    cases["one_base_exon_and_zero"] = (
        gff([("c1", "mRNA", 1, 900, "ID=t1;Parent=g1"), ("c1", "exon", 7, 7, "ID=e1;Parent=t1"), ("c1", "exon", 0, 0, "ID=e2;Parent=t1"),
             ("c1", "exon", "+20", "+21", "ID=e3;Parent=t1")]),
        HEADER + "".join(f"G,c1,{s},{s}\n" for s in ("-1", "0", "1", "6", "7", "8", "+20", "21", "22", "-0")))
    return cases


ANNOTATION_OVER_BOWTIE = gff([
    ("chrA", "gene", 1, 1977, "ID=gA"),
    ("chrA", "mRNA", 150, 900, "ID=a1;Parent=gA"),
    ("chrA", "exon", 150, 240, "ID=a1e1;Parent=a1"),
    ("chrA", "exon", 270, 420, "ID=a1e2;Parent=a1"),
    ("chrA", "exon", 600, 900, "ID=a1e3;Parent=a1"),
    ("chrA", "mRNA", 200, 1200, "ID=a2;Parent=gA"),
    ("chrA", "exon", 200, 290, "ID=a2e1;Parent=a2"),
    ("chrA", "exon", 600, 1200, "ID=a2e2;Parent=a2"),
    ("chrA", "mRNA", 200, 1900, "ID=a3;Parent=gA"),
    ("chrA", "exon", 1000, 1900, "ID=a3e1;Parent=a3"),
    ("chrA", "mRNA", 1400, 1977, "ID=b1;Parent=gA2"),
    ("chrA", "exon", 1500, 1977, "ID=b1e1;Parent=b1"),
    ("chrB", "mRNA", 1, 850, "ID=c1;Parent=gB"),
    ("chrB", "exon", 1, 400, "ID=c1e1;Parent=c1"),
    ("chrB", "mRNA", 1, 850, "ID=c2;Parent=gB"),
    ("chrB", "exon", 300, 850, "ID=c2e1;Parent=c2"),
    ("chrB", "exon", 100, 350, "ID=orphan;Parent=nowhere"),
    ("chrC", "mRNA", 1, 261, "ID=d1;Parent=gC"),
    ("chrC", "exon", 50, 200, "ID=d1e1;Parent=d1"),
    # an unaligned guide is printed as '*', 0, 22: position 0 of '*' is asked, not position 1
    ("*", "mRNA", 0, 0, "ID=s1;Parent=gS"),
    ("*", "exon", 0, 0, "ID=s1e1;Parent=s1"),
    ("*", "mRNA", 1, 30, "ID=s2;Parent=gT"),
    ("*", "exon", 1, 30, "ID=s2e1;Parent=s2"),
    ("*", "mRNA", 1, 30, "ID=s3;Parent=gT"),
])


def load_reference(root):
    path = pathlib.Path(root) / "src" / "crackling" / "utils" / "countHitTranscripts.py"
    spec = importlib.util.spec_from_file_location("reference_countHitTranscripts", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sample_of(ref, tmp):
    """The reference's own sample, taken from the files useSampleData() writes."""
    with contextlib.redirect_stdout(io.StringIO()):
        annotation, crackling = ref.useSampleData()
    # the writers are left open by the reference: flush them through their names
    import gc
    gc.collect()
    a, c = pathlib.Path(annotation), pathlib.Path(crackling)
    texts = a.read_text(), c.read_text()
    a.unlink()
    c.unlink()
    return texts


def run_reference(ref, annotation, crackling):
    """-> the bytes the reference writes, or None when it raises."""
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        shutil.copy(annotation, tmp / "annotation.gff")
        shutil.copy(crackling, tmp / "crackling.csv")
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                results = ref.process(str(tmp / "annotation.gff"), str(tmp / "crackling.csv"))
        except Exception:
            return None
        with open(tmp / "out.csv", "w") as fp:
            writer = csv.writer(fp, delimiter=",", quotechar='"', dialect="unix", quoting=csv.QUOTE_MINIMAL)
            for r in results:
                writer.writerow(r)
        return (tmp / "out.csv").read_bytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    if OUT.exists():
        shutil.rmtree(OUT)
    OUT.mkdir(parents=True)
    listing = []
    with tempfile.TemporaryDirectory() as tmp:
        cases = case_list(sample_of(ref, tmp))
    for name, (annotation, crackling) in cases.items():
        d = OUT / name
        d.mkdir()
        (d / "annotation.gff").write_bytes(annotation.encode())
        (d / "crackling.csv").write_bytes(crackling.encode())
        entry = {"name": name, "annotation": f"{name}/annotation.gff", "crackling": f"{name}/crackling.csv"}
        got = run_reference(ref, d / "annotation.gff", d / "crackling.csv")
        if got is None:
            entry["error"] = True
        else:
            (d / "expected.csv").write_bytes(got)
            entry["expected"] = f"{name}/expected.csv"
        assert name.startswith("error_") == (got is None), name
        listing.append(entry)
    d = OUT / "bowtie"
    d.mkdir()
    (d / "annotation.gff").write_bytes(ANNOTATION_OVER_BOWTIE.encode())
    for cfg in json.loads((BOWTIE / "configs.json").read_text()):
        got = run_reference(ref, d / "annotation.gff", BOWTIE / f"{cfg['name']}.csv")
        assert got is not None, cfg["name"]
        (d / f"{cfg['name']}.expected.csv").write_bytes(got)
        listing.append({"name": f"bowtie_{cfg['name']}", "annotation": "bowtie/annotation.gff",
                        "crackling": f"../bowtie/{cfg['name']}.csv", "expected": f"bowtie/{cfg['name']}.expected.csv"})
    (OUT / "cases.json").write_text(json.dumps(listing, indent=1) + "\n")
    print(f"{len(listing)} cases, {sum(1 for e in listing if e.get('error'))} of them errors")


if __name__ == "__main__":
    main()
