#!/usr/bin/env python3
"""Recipe of tests/golden/bowtie/: a genome of a few kbp, an input FASTA cut out of it and what the reference's own run
(src/crackling/Crackling.py, the "Bowtie analysis" :600-725 and the off-target scoring behind it) makes of the input's
guides under six configurations: optimisation ultralow, medium and high, each with [bowtie2] page-length 0 and 7, n = 2.

Neither Bowtie2 nor an index of it is to be had, so [bowtie2] binary names a stand-in written to a temporary directory: a
brute-force exact matcher over the genome FASTA that [input] bowtie2-index points at.  For every read it prints one SAM
line.  With occurrences (the read itself on strand 0, its reverse complement on strand 1; windows inside one record, no
N): flag 0 or 16, the record's name up to the first blank, the 1-based position of the first occurrence in (record, pos,
strand) order, SEQ as Bowtie2 prints it (reverse-complemented on strand 1), XM:i:0, and XS:i:0 when a second occurrence
exists.  Without: an unaligned line (flag 4, *, 0, no XM).  The reference removes Bowtie's output between pages, so the
stand-in appends every page to a file of its own, which is kept, compressed, as <config>.sam.gz.  RNAfold's stand-in is the one of
tools/make_golden_consensus.py; what it printed at ultralow is fold.txt.gz.

Off-target scoring is enabled: the reference's extractOfftargets.py lists the genome's sites, oracle/_ref/isslCreateIndex
turns them into index.issl and oracle/_ref/isslScoreOfftargets scores (build both with `make -C oracle ref`).

genome.fa is built so that the input holds a guide of every kind KINDS lists; the recipe checks that against the CSVs,
the SAMs and a brute-force count of its own, and fails otherwise.  Data only: nothing of the reference's text is copied.
Never imported by a test."""
import argparse
import csv
import gzip
import json
import os
import pathlib
import random
import shutil
import stat
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import make_golden_consensus as mgc  # noqa: E402

OUT = ROOT / "tests" / "golden" / "bowtie"
PAMS = ["AGG", "CGG", "GGG", "TGG", "AAG", "CAG", "GAG", "TAG"]
COLUMNS = ["seq", "isUnique", "consensusCount", "passedBowtie", "bowtieChr", "bowtieStart", "bowtieEnd", "mitOfftargetscore", "cfdOfftargetscore",
                         "passedOffTargetScore"]
CONFIGS = [dict(mgc.config(f"{opt}_page{page}", opt, 2), page_length=page, score_threshold=75, max_distance=4, method="and")
           for opt in ("ultralow", "medium", "high") for page in (0, 7)]
KINDS = ["accepted, read 0 aligned", "accepted, read 0 unaligned", "rejected by two variants once each",
         "rejected by one variant twice on one strand", "rejected by one variant once per strand",
         "an occurrence with one mismatch does not count", "a window across a record boundary does not count",
         "two guides of a page share a 20-mer: the earlier one untested", "the same two guides in two pages: both tested",
         "rejected by Bowtie and never scored (medium, high)"]

CONFIG = """[general]
name = golden
optimisation = {optimisation}
[consensus]
n = {n}
mm10db = {mm10db}
sgrnascorer2 = {sgrnascorer2}
chopchop = {chopchop}
[input]
exon-sequences = {inputs}
offtarget-sites = {issl}
gff-annotation = unused
bowtie2-index = {genome}
batch-size = 5000000
[output]
dir = {outdir}
filename = guides.txt
delimiter = ,
[offtargetscore]
enabled = True
binary = {scorer}
method = {method}
threads = 1
page-length = 5000000
score-threshold = {score_threshold}
max-distance = {max_distance}
[sgrnascorer2]
model = {model}
score-threshold = {sgrna_threshold}
[bowtie2]
binary = {bowtie}
threads = 1
page-length = {page_length}
[rnafold]
binary = {rnafold}
threads = 1
page-length = 5000000
low_energy_threshold = {low_energy}
high_energy_threshold = {high_energy}
"""

# argv: -x <genome FASTA> -p <threads> --reorder --no-hd -t -r -U <reads> -S <output>
BOWTIE_STAND_IN = """#!{python}
import sys
sys.path.insert(0, {tools!r})
import make_golden_bowtie
make_golden_bowtie.stand_in(sys.argv)
"""

rc = mgc.rc


# ---- the stand-in ----------------------------------------------------------------------------------------------------

def read_records(path):
    """-> [(name up to the first blank, upper-cased sequence)]"""
    records = []
    for line in pathlib.Path(path).read_text().splitlines():
        if line.startswith(">"):
            records.append([line[1:].split()[0] if line[1:].split() else "", []])
        elif records:
            records[-1][1].append(line.strip().upper())
    return [(name, "".join(parts)) for name, parts in records]


def occurrences(records, read):
    """(record, pos, strand) of every occurrence of `read`, ascending."""
    found = []
    for strand, text in ((0, read), (1, rc(read))):
        for r, (_, seq) in enumerate(records):
            at = seq.find(text)
            while at >= 0:
                found.append((r, at, strand))
                at = seq.find(text, at + 1)
    return sorted(found)


def sam_line(records, k, read):
    occ = occurrences(records, read)
    qual = "I" * len(read)
    if not occ:
        return f"{k}\t4\t*\t0\t0\t*\t*\t0\t0\t{read}\t{qual}\tYT:Z:UU"
    r, pos, strand = occ[0]
    second = "XS:i:0\t" if len(occ) > 1 else ""
    return (f"{k}\t{16 * strand}\t{records[r][0]}\t{pos + 1}\t{1 if len(occ) > 1 else 42}\t{len(read)}M\t*\t0\t0\t"
            f"{rc(read) if strand else read}\t{qual}\tAS:i:0\t{second}XN:i:0\tXM:i:0\tXO:i:0\tXG:i:0\tNM:i:0\tMD:Z:{len(read)}\tYT:Z:UU")


def stand_in(argv):
    records = read_records(argv[argv.index("-x") + 1])
    reads = pathlib.Path(argv[argv.index("-U") + 1]).read_text().split()
    text = "".join(sam_line(records, k, read) + "\n" for k, read in enumerate(reads))
    pathlib.Path(argv[argv.index("-S") + 1]).write_text(text)
    with open("bowtie_output.seen", "a") as fh:
        fh.write(text)


# ---- the genome ------------------------------------------------------------------------------------------------------

def make_genome():
    """-> (genome FASTA, input FASTA, planted: kind -> the 23-mers of the input planted for it)"""
    rnd = random.Random(20261018)
    rand = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))  # noqa: E731
    planted = {k: [] for k in ("two variants", "twice one strand", "once per strand", "one mismatch", "boundary", "shared")}
    region, second = [rand(60)], [rand(50)]

    def body():
        while True:  # no run of four T: most such guides would fail the consensus, and these have to reach the scorer too
            x = rnd.choice("ACG") + rand(18) + "G"
            if "TTTT" not in x and 8 <= sum(c in "AT" for c in x) <= 12:
                return x

    for _ in range(3):
        x = body()
        planted["two variants"].append(x + "AGG")
        region += ["A" + x + "AGG", rand(rnd.randrange(30, 46))]
        second += ["T" + x + "TAG", rand(rnd.randrange(15, 40))]
        x = body()
        planted["twice one strand"].append(x + "CGG")
        region += ["A" + x + "CGG", rand(rnd.randrange(30, 46))]
        second += ["T" + x + "CGG", rand(rnd.randrange(15, 40))]
        x = body()
        planted["once per strand"].append(x + "GGG")
        region += ["A" + x + "GGG", rand(rnd.randrange(30, 46))]
        second += ["T" + rc(x + "GGG"), rand(rnd.randrange(15, 40))]
        x = body()
        planted["one mismatch"].append(x + "TGG")
        region += ["A" + x + "TGG", rand(rnd.randrange(30, 46))]
        second += ["T" + x[:9] + rc(x[9]) + x[10:] + "TGG", rand(rnd.randrange(15, 40))]
    shared = [body() for _ in range(2)]
    for z in shared:  # the earlier guide of each pair ...
        planted["shared"].append((z + "AGG", z + "CGG"))
        region += ["A" + z + "AGG", rand(rnd.randrange(30, 46))]
    edge = [body() + "AGG", body() + "TGG"]
    planted["boundary"] = edge
    region += ["A" + edge[0], rand(40), "NNNNNNNN", rand(30), "A" + edge[1], rand(40)]
    lower = rand(60).lower()
    region += [lower, rand(420)]
    for z in shared:  # ... and the later one, more than a page of seven behind it
        region += ["A" + z + "CGG", rand(rnd.randrange(30, 46))]
    region = "".join(region)
    chr_a = rand(150) + region + rand(120) + edge[0][:12]              # ends inside edge[0] ...
    tiny = edge[0][12:] + rand(11)                                        # ... which goes on in a record of 22 bases
    chr_b = "".join(second) + "ACGTNNNNNNNNNNACGT" + rand(60).lower() + rand(100) + edge[1][:12]
    chr_c = edge[1][12:] + rand(250)
    assert len(tiny) == 22
    genome = (">chrA first record\n" + mgc.wrap(chr_a) + ">tiny of 22 bases\n" + mgc.wrap(tiny) + ">chrB second copies\n" + mgc.wrap(chr_b, 70) +
              ">chrC\n" + mgc.wrap(chr_c))
    at = chr_a.index(region)
    return genome, ">exons chrA:%d-%d\n" % (at + 1, at + len(region)) + mgc.wrap(region), planted


# ---- the reference ---------------------------------------------------------------------------------------------------

def executable(path, text):
    path.write_text(text)
    path.chmod(path.stat().st_mode | stat.S_IXUSR)
    return path


def run_reference(reference, cfg, genome, fasta, issl, work):
    """-> (rows of COLUMNS as dicts, the SAM of all pages, what RNAfold's stand-in printed)"""
    work = pathlib.Path(work)
    outdir = work / "out"
    outdir.mkdir()
    rnafold = executable(work / "rnafold_stand_in", mgc.STAND_IN.format(python=sys.executable))
    bowtie = executable(work / "bowtie_stand_in", BOWTIE_STAND_IN.format(python=sys.executable, tools=str(ROOT / "tools")))
    ini = work / "golden.ini"
    ini.write_text(CONFIG.format(inputs=fasta, genome=genome, issl=issl, outdir=outdir, rnafold=rnafold, bowtie=bowtie,
                                 scorer=ROOT / "oracle" / "_ref" / "isslScoreOfftargets",
                                 model=pathlib.Path(reference) / "src" / "crackling" / "utils" / "data" / "model-py3.txt",
                                 **{k: v for k, v in cfg.items() if k != "name"}))
    driver = work / "driver.py"
    driver.write_text(mgc.DRIVER)
    env = dict(os.environ, PYTHONPATH=str(pathlib.Path(reference) / "src"))
    r = subprocess.run([sys.executable, str(driver), str(ini)], env=env, capture_output=True, text=True, cwd=work)
    errlog = outdir / "golden-golden.errlog"
    if r.returncode:
        raise RuntimeError(f"reference failed on {cfg['name']}:\n{r.stdout}\n{r.stderr}\n{errlog.read_text() if errlog.exists() else ''}")
    with open(outdir / "golden-guides.txt", newline="") as fh:
        rows = [{c: row[c] for c in COLUMNS} for row in csv.DictReader(fh, delimiter=",", quotechar='"')]
    seen = work / "bowtie_output.seen"
    fold = work / "RNAfold_output.seen"
    return rows, seen.read_text() if seen.exists() else "", fold.read_text() if fold.exists() else ""


def build_index(reference, genome, work):
    """genome FASTA -> (the reference's sorted site list, .issl of it)"""
    work = pathlib.Path(work)
    sites, issl = work / "offtargets.txt", work / "index.issl"
    env = dict(os.environ, PYTHONPATH=str(pathlib.Path(reference) / "src"))
    subprocess.run([sys.executable, "-m", "crackling.utils.extractOfftargets", "--threads", "1", str(sites), str(genome)], env=env,
                   check=True, capture_output=True, cwd=work)
    subprocess.run([str(ROOT / "oracle" / "_ref" / "isslCreateIndex"), str(sites), "20", "8", str(issl)], check=True,
                   capture_output=True)
    return sites, issl


# ---- the checks ------------------------------------------------------------------------------------------------------

def check_kinds(results, records, planted):
    """results: config name -> (rows, sam).  Every kind of KINDS is in the fixture."""
    seen = set()
    rows0 = {r["seq"]: r for r in results["ultralow_page0"][0]}
    rows7 = {r["seq"]: r for r in results["ultralow_page7"][0]}
    count = lambda g: {v: occurrences(records, g[:20] + pam) for v, pam in enumerate(PAMS)}  # noqa: E731
    for r in rows0.values():
        if r["passedBowtie"] == "1":
            seen.add(KINDS[0] if r["bowtieChr"] != "*" else KINDS[1])
            assert (r["bowtieChr"], r["bowtieStart"], r["bowtieEnd"]) != ("*", "0", "0")
    for g in planted["two variants"]:
        occ = count(g)
        assert [len(occ[v]) for v in range(8)] == [1, 0, 0, 0, 0, 0, 0, 1] and rows0[g]["passedBowtie"] == "0", g
        seen.add(KINDS[2])
    for g in planted["twice one strand"]:
        occ = count(g)
        assert [len(occ[v]) for v in range(8)] == [0, 2, 0, 0, 0, 0, 0, 0] and {s for _, _, s in occ[1]} == {0}, g
        assert rows0[g]["passedBowtie"] == "0" and rows0[g]["bowtieChr"] == "*"
        seen.add(KINDS[3])
    for g in planted["once per strand"]:
        occ = count(g)
        assert [len(occ[v]) for v in range(8)] == [0, 0, 2, 0, 0, 0, 0, 0] and {s for _, _, s in occ[2]} == {0, 1}, g
        assert rows0[g]["passedBowtie"] == "0"
        seen.add(KINDS[4])
    genome_text = "\n".join(seq for _, seq in records)
    for g in planted["one mismatch"]:
        near = g[:9] + rc(g[9]) + g[10:]
        assert near in genome_text and sum(len(o) for o in count(g).values()) == 1 and rows0[g]["passedBowtie"] == "1", g
        seen.add(KINDS[5])
    joined = "".join(seq for _, seq in records)
    for g in planted["boundary"]:
        assert joined.count(g) == 2 and sum(len(o) for o in count(g).values()) == 1 and rows0[g]["passedBowtie"] == "1", g
        seen.add(KINDS[6])
    order0 = [r["seq"] for r in results["ultralow_page0"][0]]
    for early, late in planted["shared"]:
        assert order0.index(early) // 7 < order0.index(late) // 7
        assert [rows0[early][c] for c in COLUMNS[-7:-3]] == ["?"] * 4 and rows0[late]["passedBowtie"] == "0", early
        seen.add(KINDS[7])
        assert rows7[early]["passedBowtie"] == "0" and rows7[late]["passedBowtie"] == "0", early
        seen.add(KINDS[8])
    for name in ("medium_page0", "medium_page7", "high_page0", "high_page7"):
        rows = results[name][0]
        assert any(r["passedBowtie"] == "0" and r["passedOffTargetScore"] == "?" and r["mitOfftargetscore"] == "?" for r in rows), name
        assert any(r["passedBowtie"] == "1" and r["passedOffTargetScore"] != "?" for r in rows), name
        assert not any(r["passedBowtie"] == "0" and r["passedOffTargetScore"] != "?" for r in rows), name
    seen.add(KINDS[9])
    assert any(r["passedBowtie"] == "0" and r["mitOfftargetscore"] != "?" for r in rows0.values()), "ultralow scores the rejected too"
    # the reference's look-up by printed sequence: the strand-1 guide of a window CCT N{18} NGG hands its verdict over
    assert any(r["passedBowtie"] == "?" and rc(g).startswith("CCT") and rows0.get(rc(g), {}).get("passedBowtie", "?") != "?"
               for g, r in rows0.items()), "no CCT ... NGG window among the guides"
    assert seen == set(KINDS), sorted(set(KINDS) - seen)
    return seen


def make_goldens(reference):
    if OUT.exists():
        shutil.rmtree(OUT)
    OUT.mkdir(parents=True)
    genome_text, input_text, planted = make_genome()
    genome, fasta = OUT / "genome.fa", OUT / "input.fa"
    genome.write_text(genome_text)
    fasta.write_text(input_text)
    records = read_records(genome)
    assert len(records) >= 3 and any(len(seq) < 23 for _, seq in records) and 2000 < sum(len(seq) for _, seq in records) < 5000
    assert any(c.islower() for c in genome_text.split("\n", 1)[1]) and "NNNN" in genome_text
    with tempfile.TemporaryDirectory() as work:
        sites, issl = build_index(reference, genome, work)
        shutil.copyfile(issl, OUT / "index.issl")
    results = {}
    for cfg in CONFIGS:
        with tempfile.TemporaryDirectory() as work:
            rows, sam, fold = run_reference(reference, cfg, genome, fasta, OUT / "index.issl", work)
        results[cfg["name"]] = (rows, sam)
        with open(OUT / f"{cfg['name']}.csv", "w", newline="") as fh:
            w = csv.DictWriter(fh, COLUMNS, dialect="unix", quoting=csv.QUOTE_MINIMAL)
            w.writeheader()
            w.writerows(rows)
        with open(OUT / f"{cfg['name']}.sam.gz", "wb") as fh:  # eight lines per guide: kept compressed, no time stamp inside
            fh.write(gzip.compress(sam.encode(), 9, mtime=0))
        if cfg["name"] == "ultralow_page0":
            (OUT / "fold.txt.gz").write_bytes(gzip.compress(fold.encode(), 9, mtime=0))
            assert 200 <= len(rows) <= 320, len(rows)
        tested = sum(r["passedBowtie"] != "?" for r in rows)
        print(cfg["name"], len(rows), "guides,", len(sam.splitlines()) // 8, "in the Bowtie step,", tested, "tested,",
              sum(r["passedBowtie"] == "0" for r in rows), "rejected,", sum(r["mitOfftargetscore"] != "?" for r in rows), "scored")
    check_kinds(results, records, planted)
    (OUT / "configs.json").write_text("[\n" + ",\n".join(json.dumps(c) for c in CONFIGS) + "\n]\n")
    for f in sorted(OUT.iterdir()):
        assert f.stat().st_size < 1 << 20, f
        print(f"{f.stat().st_size:8d} {f.name}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default="/root/reference")
    make_goldens(ap.parse_args().reference)
