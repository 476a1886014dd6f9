"""CPU: the host model of RNAfold's exchange (tests/folds_util.py) pinned to the package's two Python helpers on every golden
fold text and on every crafted answer that holds none of the bytes they part from the reference on, and the shared rules of
crackling_amd/csrc/issl_folds_text.hpp -- the code the kernels run per row -- run as a stand-alone program under
AddressSanitizer + UBSan (tools/folds_sanitize.cpp) against the model on every crafted answer."""
import gzip
import pathlib
import struct
import subprocess

import numpy as np
import pytest

import folds_util as fu

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
GOLDEN_TEXTS = ["bowtie/fold.txt.gz", "results/headers_fold.txt.gz"]
GUIDES = fu.random_guides(300)
CASES = fu.crafted_cases(GUIDES)


def golden_text(name):
    return gzip.decompress((GOLDEN / name).read_bytes())


def guides_of(text):
    """The guides a golden fold text answers (G + guide[1:20] + the scaffold: the first base is not in it), some that it does
    not, and the order shuffled."""
    lines = text.decode().splitlines()[0::2]
    guides = ["A" + l[1:20].replace("U", "T") + "AGG" for l in lines if len(l) >= 20] + fu.random_guides(25, seed=5)
    return [guides[i] for i in np.random.default_rng(4).permutation(len(guides))]


def same_as_helpers(text_bytes, guides):
    import crackling_amd as ca
    folds, texts = fu.model(text_bytes, guides)
    text = text_bytes.decode("latin-1")
    assert ca.read_rnafold_output(text, guides).tobytes() == folds.tobytes()
    assert ca.read_rnafold_text(text, guides) == texts
    return folds, texts


@pytest.mark.parametrize("name", GOLDEN_TEXTS)
def test_model_equals_the_helpers_on_the_golden_fold_texts(name):
    import crackling_amd as ca
    assert ca.Folds is ca.folds.Folds and ca.folds.LINE_BYTES == 101 and fu.SCAFFOLD == ca.SCAFFOLD
    text = golden_text(name)
    assert not fu.differs(text)
    guides = guides_of(text)
    folds, texts = same_as_helpers(text, guides)
    assert folds["present"].sum() > 20 and (folds["scaffold"] == 1).any() and (folds["present"] == 0).any()
    assert any(t is not None and t[2] == "" for t in texts) and any(t is None for t in texts)
    twenty = [g[:20] for g in guides]
    assert fu.model(text, twenty)[0].tobytes() == folds.tobytes()


def test_the_crafted_answers_say_what_they_are_named_for():
    import crackling_amd as ca
    assert "rnafold_reader" in ca.pipeline.batches.__doc__ and "float(x.strip())" in ca.pipeline.batches.__doc__  # where the readers part
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names) > 100
    by = {name: (text, code) for name, text, code in CASES}
    for name, (text, code) in by.items():
        if code is None:
            folds, texts = fu.model(text, GUIDES)
            if not fu.differs(text):
                same_as_helpers(text, GUIDES)
        else:
            with pytest.raises(fu.Refused) as e:
                fu.model(text, GUIDES)
            assert e.value.code == code, name
    n = len(GUIDES)
    folds, texts = fu.model(by["every pair"][0], GUIDES)
    assert folds["present"].all() and {0, 1} == set(folds["scaffold"].tolist())
    assert {-30.0, -30.01, -29.99, -18.0, -18.01, -17.99} <= set(folds["energy"].tolist())
    assert fu.model(by["shuffled"][0], GUIDES)[0].tobytes() == folds.tobytes()
    assert fu.model(by["a superset"][0], GUIDES)[0].tobytes() == folds.tobytes()
    assert fu.model(by["U and T mixed inside a key"][0], GUIDES)[0].tobytes() == folds.tobytes()
    for name in ("CR LF", "lone CR", "line ends mixed", "no final terminator", "two blank lines give it back", "an odd line count",
                 "an odd line count, open"):
        assert fu.model(by[name][0], GUIDES)[0].tobytes() == folds.tobytes(), name
    assert fu.model(by["missing pairs"][0], GUIDES)[0]["present"].tolist() == [1 if k % 3 else 0 for k in range(n)]
    assert not fu.model(by["a blank line shifts the parity"][0], GUIDES)[0]["present"].any()
    assert fu.model(by["a blank line in the middle"][0], GUIDES)[0]["present"].tolist() == [1] * 20 + [0] * (n - 20)
    later, _ = fu.model(by["duplicates, the later wins"][0], GUIDES)
    assert [round(x, 2) for x in later["energy"][:10]] == [-7.0 - k / 100 for k in range(10)] and later["scaffold"][:10].tolist() == [0] * 10
    assert [round(x, 2) for x in later["energy"][10:20]] == [-31.0 - k / 100 for k in range(10)] and later["scaffold"][10:20].tolist() == [1] * 10
    assert not fu.model(by["first lines under 20 bytes"][0], GUIDES)[0]["present"][:19].any()
    assert fu.model(by["first lines under 20 bytes"][0], GUIDES)[0]["present"][30] == 1
    assert fu.model(by["first lines of 20 bytes"][0], GUIDES)[0]["present"][:8].all()
    assert not fu.model(by["lower case matches nothing"][0], GUIDES)[0]["present"][:5].any()
    for c in fu.STRIP_BYTES:
        f, t = fu.model(by["trailing 0x%02x" % c][0], GUIDES)
        assert f[:12].tobytes() == folds[:12].tobytes() and all(x[0] == fu.first_line(g) for x, g in zip(t[:12], GUIDES)), c
    f, t = fu.model(by["trailing bytes that are no blanks"][0], GUIDES)
    assert t[0][0].endswith("\x85") and f["present"][:6].all()
    f, _ = fu.model(by["the scaffold at s > 0"][0], GUIDES)
    assert f["scaffold"][0:40:3].all() and [round(x, 2) for x in f["energy"][0:40:3]] == [-26.0 - k / 100 for k in range(0, 40, 3)]
    f, _ = fu.model(by["TAB before the parenthesis, with a blank"][0], GUIDES)
    assert f[:2].tolist() == [(-27.1, 1, 1), (-3.1, 0, 1)]
    f, _ = fu.model(by["separators as the blank of the patterns"][0], GUIDES)
    assert f[7:10].tolist() == [(-3.25, 0, 1), (-4.5, 1, 1), (-1.5, 0, 1)]
    f, _ = fu.model(by["a near miss at every literal position"][0], GUIDES)
    assert f["scaffold"][:52].tolist() == [0] * 51 + [1] and f["present"][:52].all()
    assert [round(x, 2) for x in f["energy"][:51]] == [-33.0 - k / 100 for k in range(51)]
    f, t = fu.model(by["number forms"][0], GUIDES)
    assert f["energy"][:16].tolist() == [-5.3, -5.3, 5.0, 0.5, 7.5, 123456789.012345, -0.0, 1e-15, 0.5, -5.3, 999999999999999.0, 0.0, -0.0,
                                         7.0, 5e-15, 1e14]
    assert np.signbit(f["energy"][6]) and np.signbit(f["energy"][12]) and f["present"][:16].all()
    f, t = fu.model(by["two blanks behind the structure"][0], GUIDES)
    assert [x[2] for x in t[:5]] == ["", "", "", "", ""] and f["present"][:5].all() and f["scaffold"][4] == 0
    f, t = fu.model(by["no pattern matches: texts without a fold"][0], GUIDES)
    assert not f["present"][:5].any() and f[:5].tobytes() == bytes(80) and all(x is not None for x in t[:5])
    assert t[0] == (fu.first_line(GUIDES[0]), "....", "5.3") and t[4] == (fu.first_line(GUIDES[4]), "", "")
    with pytest.raises(fu.Refused) as e:
        fu.model(by["the lowest refused row is named"][0], GUIDES)
    assert (e.value.code, e.value.row) == (fu.FORMAT, 20)
    assert fu.model(by["faults nobody looks up"][0], GUIDES)[0].tobytes() == folds.tobytes()
    assert fu.model(by["a refused pair replaced by a later one"][0], GUIDES)[0].tobytes() == folds.tobytes()
    for name in ("no text", "one byte", "one byte, no line end", "one line"):
        f, t = fu.model(by[name][0], GUIDES)
        assert not f["present"].any() and t == [None] * n, name
    f, t = fu.model(by["a first line of 100 KB"][0], GUIDES)
    assert len(t[0][0]) == 100100 and f["present"][:5].all()
    f, t = fu.model(by["a second line of 100 KB"][0], GUIDES)
    assert f[0].tolist() == (-41.25, 1, 1) and len(t[0][1]) == 100100
    f, t = fu.model(by["a second line of 100 KB without the scaffold"][0], GUIDES)
    assert f[0].tolist() == (-41.5, 0, 1)


def test_number_grammar():
    header = (ROOT / "crackling_amd" / "csrc" / "issl_folds_text.hpp").read_text()  # the grammar this test restates
    assert "read_number" in header and "digits[.digits] or .digits" in header and "counted > 15" in header
    assert fu.number("-5.30") == -5.3 and fu.number(" -5.30") == -5.3 and fu.number("5.") == 5.0 and fu.number("+.5") == 0.5
    assert fu.number("007.5") == 7.5 and fu.number("123456789.012345") == 123456789.012345 and fu.number("\t1 ") == 1.0
    for bad in ("-1e2", "- 5.3", "", ".", "+", "1_0", "inf", "nan", "1 2", "\n1", "1\n", "0x1", "１"):
        assert fu.number(bad) == fu.FORMAT, bad
    assert fu.number("1234567890.123456") == fu.UNSUPPORTED and fu.number("0000000000000001.5") == 1.5
    rng = np.random.default_rng(8)
    for _ in range(20000):  # one division of two exact doubles is the correctly rounded value: float() of the same text
        digits = int(rng.integers(1, 16))
        frac = int(rng.integers(0, digits + 1))
        s = "".join(str(int(d)) for d in rng.integers(0, 10, digits))
        t = ("-" if rng.integers(0, 2) else "") + s[:digits - frac] + "." + s[digits - frac:]
        assert fu.bits(fu.number(t)) == fu.bits(float(t)), t


def write_cases(path, cases, guides):
    with open(path, "wb") as out:
        for _, text, _ in cases:
            out.write(struct.pack("<I", len(guides)) + "".join(guides).encode() + struct.pack("<Q", len(text)) + text)


def expected_output(cases, guides):
    out = []
    for k, (_, text, code) in enumerate(cases):
        out.append(f"case {k}")
        try:
            folds, texts = fu.model(text, guides)
        except fu.Refused as e:
            out.append(f"refused {e.code} {e.row}")
            continue
        for f, t in zip(folds, texts):
            if t is None:
                out.append("-")
            else:
                out.append("%016x %d %d " % (fu.bits(f["energy"]), f["scaffold"], f["present"]) + " ".join(t))
    return out


def test_shared_rules_under_asan_and_ubsan_equal_the_model(tmp_path):
    """tools/folds_sanitize.cpp: every crafted answer and both golden texts through the header the kernels include, as a
    stand-alone CPU program; its folds and the texts its spans cut out must be the model's."""
    exe = tmp_path / "folds_sanitize"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            str(ROOT / "tools" / "folds_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    sets = [(CASES, GUIDES)]
    for name in GOLDEN_TEXTS:
        text = golden_text(name)
        sets.append(([(name, text, None), (name + " cut", text[:len(text) // 2 + 7], None)], guides_of(text)))
    for k, (cases, guides) in enumerate(sets):
        path = tmp_path / f"cases{k}.bin"
        write_cases(path, cases, guides)
        run = subprocess.run([str(exe), str(path)], capture_output=True,
                             env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
        assert run.returncode == 0 and b"ERROR" not in run.stderr, run.stderr.decode(errors="replace")[-4000:]
        got = run.stdout.decode("latin-1").split("\n")[:-1]
        # the program prints spans; cut them out of the case's text
        want = expected_output(cases, guides)
        lines, case_text = [], None
        at = -1
        for line in got:
            if line.startswith("case "):
                at += 1
                case_text = cases[at][1]
                lines.append(line)
            elif line == "-" or line.startswith("refused"):
                lines.append(line)
            else:
                w = line.split(" ")
                spans = [(int(w[3 + 2 * i]), int(w[4 + 2 * i])) for i in range(3)]
                assert all(o + n <= len(case_text) for o, n in spans), (cases[at][0], line)
                lines.append(" ".join(w[:3]) + " " + " ".join(case_text[o:o + n].decode("latin-1") for o, n in spans))
        assert len(lines) == len(want)
        for a, b in zip(lines, want):
            assert a == b, (a[:300], b[:300])
