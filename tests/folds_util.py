"""Host model of RNAfold's exchange (issl_folds_* of include/issl_hip.h): Crackling.py:439-497 restated -- the lines of a
text-mode file (io.StringIO with newline=None), a dictionary of line pairs under first[1:20], the three text columns, the
two regular expressions of :396-397 -- with the number grammar of the header in place of ast.literal_eval.  Bytes are
read as latin-1, one character per byte, and blanks are the ASCII ones only, so that a byte >= 0x80 is an ordinary
character.  Nothing of the library runs here.  The crafted answers below are shared by the CPU tests (against
tools/folds_sanitize.cpp) and the GPU tests."""
import io
import re
import struct

import numpy as np

FOLD_DTYPE = np.dtype([("energy", "<f8"), ("scaffold", "<u4"), ("present", "<u4")])
SCAFFOLD = "GUUUUAGAGCUAGAAAUAGCAAGUUAAAAUAAGGCUAGUCCGUUAUCAACUUGAAAAAGUGGCACCGAGUCGGUGCUUUU"
WS = "\t\n\x0b\x0c\r\x1c\x1d\x1e\x1f "
STRIP_BYTES = [9, 10, 11, 12, 13, 0x1c, 0x1d, 0x1e, 0x1f, 0x20]
DIFFERING = set(b"\x0b\x0c\x1c\x1d\x1e") | set(range(0x80, 0x100))  # where str.splitlines() / str.rstrip() part from the reference
LIT1, LIT2 = "((((....))))...))))", "((((....))))(((((((...)))))))..."
_S = r"[\t-\r\x1c-\x20]"
_SCAFFOLD_FOLD = re.compile(".{28}" + re.escape(LIT1) + ".{21}" + re.escape(LIT2) + _S + r"\((.+)\)")
_ENERGY = re.compile(_S + r"\((.+)\)")
_NUMBER = re.compile(r"[ \t]*([+-]?)(?:([0-9]+)(?:\.([0-9]*))?|\.([0-9]+))[ \t]*\Z")
FORMAT, UNSUPPORTED = -3, -4  # ISSL_E_FORMAT, ISSL_E_UNSUPPORTED


class Refused(Exception):
    def __init__(self, code, row):
        super().__init__(f"[{code}] row {row}")
        self.code, self.row = code, row


def number(text):
    """The header's number grammar -> float, or FORMAT / UNSUPPORTED."""
    m = _NUMBER.match(text)
    if not m:
        return FORMAT
    sign, whole, frac, bare = m.groups()
    whole, frac = (whole or ""), (frac or "") + (bare or "")
    if len(whole.lstrip("0")) + len(frac) > 15:
        return UNSUPPORTED
    value = float(int(whole + frac)) / float(10 ** len(frac))
    return -value if sign == "-" else value


def model(text_bytes, guides):
    """RNAfold's output (bytes) and the guides of one page (23-mers or 20-mers, in the order of the fold list) ->
    (FOLD_DTYPE array, [None | (ssL1, ssStructure, ssEnergy)]); Refused(code, lowest row) where the header refuses."""
    text = bytes(text_bytes).decode("latin-1")
    structures = {}
    first = None
    for i, line in enumerate(io.StringIO(text, newline=None)):  # :439-455
        if i % 2 == 0:
            first = line.rstrip(WS)
        else:
            structures[first[0:20][1:20].replace("U", "T")] = [first, line.rstrip(WS)]
    folds = np.zeros(len(guides), dtype=FOLD_DTYPE)
    texts = []
    for k, g in enumerate(guides):
        key = g[0:20][1:20]
        if key not in structures:  # :459
            texts.append(None)
            continue
        l1, l2 = structures[key]
        words = l2.split(" ")
        if len(words) < 2:
            raise Refused(FORMAT, k)  # (IndexError at :472)
        texts.append((l1, words[0], words[1][1:-1]))
        m = _SCAFFOLD_FOLD.search(l2)
        e = m or _ENERGY.search(l2)
        if not e:
            continue
        value = number(e.group(1))
        if not isinstance(value, float):
            raise Refused(value, k)
        folds[k] = (value, 1 if m else 0, 1)
    return folds, texts


def differs(text_bytes):
    """Does the text hold a byte on which the package's Python helpers part from the reference?"""
    return bool(DIFFERING & set(bytes(text_bytes)))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


# ---- crafted answers ---------------------------------------------------------------------------------------------------

def first_line(g, u=True):
    key = g[1:20]
    return "G" + (key.replace("T", "U") if u else key) + SCAFFOLD


def scaffold_line(num="-25.50", lead="", ws=" ", free="."):
    return lead + free * 28 + LIT1 + free * 21 + LIT2 + ws + "(" + num + ")"


def plain_line(num="-5.30", structure=".((((....))))..(((...)))...."):
    return structure + " (" + num + ")"


def pairs_text(pairs, end="\n"):
    return "".join(a + end + b + end for a, b in pairs).encode("latin-1")


def random_guides(n, seed=1):
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        g = "".join(rng.choice(list("ACGT"), 23))
        if g[1:20] not in seen:
            seen.add(g[1:20])
            out.append(g)
    return out


def default_pairs(guides, seed=2):
    """One pair per guide: scaffold and plain second lines, energies on and around both thresholds."""
    rng = np.random.default_rng(seed)
    nums = ["-30.00", "-30.01", "-29.99", "-18.00", "-18.01", "-17.99", "-5.30", " -5.30", "-25.50", "0.00"]
    out = []
    for k, g in enumerate(guides):
        num = nums[int(rng.integers(0, len(nums)))]
        out.append((first_line(g), scaffold_line(num) if rng.integers(0, 2) else plain_line(num)))
    return out


def crafted_cases(guides, group=64):
    """guides: at least 60 23-mers with distinct [1:20].  -> [(name, text bytes, None | the code a read is refused with)].
    `group`: the bytes per group of the device's line marking, for the cases that place line ends around its edges."""
    assert len(guides) >= 60 and len({g[1:20] for g in guides}) == len(guides)
    rng = np.random.default_rng(11)
    base = default_pairs(guides)
    others = random_guides(40, seed=99)
    cases = []

    def add(name, text, code=None):
        cases.append((name, text if isinstance(text, bytes) else text.encode("latin-1"), code))

    add("every pair", pairs_text(base))
    add("missing pairs", pairs_text([p for k, p in enumerate(base) if k % 3]))
    add("a superset", pairs_text(default_pairs(others[:20]) + base + default_pairs(others[20:])))
    order = rng.permutation(len(base))
    add("shuffled", pairs_text([base[i] for i in order]))
    dup = list(base) + [(first_line(g), plain_line("-7.%02d" % k)) for k, g in enumerate(guides[:30])] + \
        [(first_line(g), scaffold_line("-31.%02d" % k)) for k, g in enumerate(guides[10:20])]
    add("duplicates, the later wins", pairs_text(dup))
    add("U and T mixed", pairs_text([(first_line(g, u=bool(k % 2)), b) for k, (g, (_, b)) in enumerate(zip(guides, base))]))
    mixed = [("G" + "".join(c if rng.integers(0, 2) else c.replace("T", "U") for c in g[1:20]) + SCAFFOLD, b)
             for g, (_, b) in zip(guides, base)]
    add("U and T mixed inside a key", pairs_text(mixed))
    add("lower case matches nothing", pairs_text([(a.lower(), b) for a, b in base[:5]] + base[5:10]))
    short = [("G" + g[1:k], plain_line()) for k, g in zip(range(1, 20), guides)] + [(first_line(guides[30]), plain_line("-1.25"))]
    add("first lines under 20 bytes", pairs_text(short))
    add("first lines of 20 bytes", pairs_text([("G" + g[1:20], plain_line("-2.50")) for g in guides[:8]]))
    add("a blank line shifts the parity", b"\n" + pairs_text(base))
    add("two blank lines give it back", b"\n\n" + pairs_text(base))
    add("a blank line in the middle", pairs_text(base[:20]) + b"\r\n" + pairs_text(base[20:]))
    add("CR LF", pairs_text(base, "\r\n"))
    add("lone CR", pairs_text(base, "\r"))
    add("line ends mixed", "".join(a + ["\n", "\r\n", "\r"][k % 3] + b + ["\r", "\n", "\r\n"][k % 3] for k, (a, b) in enumerate(base)))
    add("no final terminator", pairs_text(base)[:-1])
    add("an odd line count", pairs_text(base) + first_line(guides[0]).encode() + b"\n")
    add("an odd line count, open", pairs_text(base) + first_line(guides[0]).encode())
    add("a last pair whose second line is empty", pairs_text(base[1:]) + first_line(guides[0]).encode() + b"\n\n", FORMAT)
    for c in STRIP_BYTES:
        if c in (10, 13):  # (as terminators they are the cases above; here they follow other blanks)
            t = "".join(a + " " + chr(c) + b + "\t" + chr(c) for a, b in base[:12])
        else:
            t = "".join(a + chr(c) * 2 + "\n" + b + chr(c) + " " + chr(c) + "\n" for a, b in base[:12])
        add("trailing 0x%02x" % c, t)
    add("trailing bytes that are no blanks", "".join(a + "\x85\n" + b + "\xa0\n" for a, b in base[:6]))
    add("VT, FF and separators inside lines", "".join(a + "\x0b" + "x\n" + b.replace(" (", "\x1c (", 1) + "\n" for a, b in base[:6]) +
        first_line(guides[7]) + "\n" + "..\x0c.. (-3.25)\n" + first_line(guides[8]) + "\n" + "...\x1e(-4.50)\n", FORMAT)
    add("separators as the blank of the patterns", first_line(guides[7]) + "\n" + "..\x0c.. x\x1d(-3.25)\n" + first_line(guides[8]) +
        "\n" + scaffold_line("-4.50", ws="\x1f") + " y\n" + first_line(guides[9]) + "\n" + ".... x\x0b(-1.5)\n")
    at = [(first_line(guides[k]), scaffold_line("-26.%02d" % k, lead="x" * k)) for k in range(0, 40, 3)]
    add("the scaffold at s > 0", pairs_text(at))
    add("TAB before the parenthesis", pairs_text([(first_line(guides[0]), scaffold_line("-27.10", ws="\t") + " z"),
                                                  (first_line(guides[1]), "....\t(-3.10) z"),
                                                  (first_line(guides[2]), "....\t(-3.10)")], "\n"), FORMAT)
    add("TAB before the parenthesis, with a blank", pairs_text([(first_line(guides[0]), scaffold_line("-27.10", ws="\t") + " z"),
                                                                (first_line(guides[1]), "....\t(-3.10) z")]))
    add("several closing parentheses", pairs_text([(first_line(guides[0]), "(((...))) (-1.00) (-2.00)"),
                                                   (first_line(guides[1]), scaffold_line("-28.00") + " (-9.00)"),
                                                   (first_line(guides[2]), "(((...)))) (-1.00)"),
                                                   (first_line(guides[3]), "))) ) (-6.5)")]), FORMAT)
    add("the last parenthesis closes the number", pairs_text([(first_line(guides[2]), "(((...)))) (-1.00)"),
                                                              (first_line(guides[3]), "))) ) (-6.5)"),
                                                              (first_line(guides[4]), "... ( -6.5 ) tail"),
                                                              (first_line(guides[5]), "... (-6.5")]))
    miss = []
    for k in range(51):  # one literal position flipped: the scaffold pattern misses, the energy pattern still reads
        line = list(scaffold_line("-33.%02d" % k))
        p = 28 + k if k < 19 else 68 + (k - 19)
        line[p] = "." if line[p] != "." else "("
        miss.append((first_line(guides[k]), "".join(line)))
    miss.append((first_line(guides[51]), scaffold_line("-33.99")))
    add("a near miss at every literal position", pairs_text(miss))
    add("a scaffold line that is too short behind the parenthesis", pairs_text([(first_line(guides[0]), scaffold_line("")[:-1] + ")"),
                                                                                (first_line(guides[1]), scaffold_line("1"))]))
    nums = ["-5.30", " -5.30", "5.", "+.5", "007.5", "123456789.012345", "-0.0", "0.000000000000001", "000000000000000000.5", "\t-5.30 \t",
            "999999999999999", "0", "-0", "+7", ".000000000000005", "100000000000000."]
    add("number forms", pairs_text([(first_line(g), (scaffold_line if k % 2 else plain_line)(n)) for k, (g, n) in enumerate(zip(guides, nums))]))
    add("two blanks behind the structure", pairs_text([(first_line(guides[0]), "....  (-5.30)"), (first_line(guides[1]), ".... ( -5.30)"),
                                                       (first_line(guides[2]), "....  x (-1.0)"), (first_line(guides[3]), "....   (-1.0)"),
                                                       (first_line(guides[4]), scaffold_line("-29.00").replace(" (", "  (", 1))]))
    add("a word in parentheses ahead of the energy", pairs_text([(first_line(guides[2]), ".... () (-1.0)")]), FORMAT)
    add("no pattern matches: texts without a fold", pairs_text([(first_line(guides[0]), ".... -5.30"), (first_line(guides[1]), ".... (-5.30"),
                                                                (first_line(guides[2]), ".... x)"), (first_line(guides[3]), "...( )"),
                                                                (first_line(guides[4]), " ()")]))
    # refused, and the same faults where no guide looks
    add("no blank in a looked-up second line", pairs_text(base[:9] + [(first_line(guides[9]), "....(-5.30)")] + base[10:]), FORMAT)
    add("an exponent", pairs_text(base[:40] + [(first_line(guides[40]), plain_line("-1e2"))]), FORMAT)
    add("a blank behind the sign", pairs_text([(first_line(guides[3]), scaffold_line("- 5.3"))] + base[4:]), FORMAT)
    add("sixteen digits", pairs_text(base[:5] + [(first_line(guides[5]), plain_line("1234567890.123456"))]), UNSUPPORTED)
    add("sixteen digits behind the point", pairs_text([(first_line(guides[5]), plain_line(".0000000000000001"))]), UNSUPPORTED)
    for k, n in enumerate(["inf", "1_0", "nan", "1e", " ", "+", ".", "-.", "1.2.3", "0x10", "5.3-", "--5"]):
        add("not a number: %r" % n, pairs_text(base[:k] + [(first_line(guides[k]), plain_line(n))]), FORMAT)
    add("the lowest refused row is named", pairs_text([(first_line(guides[50]), plain_line("1e5")), (first_line(guides[20]), "....(-1.0)"),
                                                       (first_line(guides[30]), plain_line("1234567890.1234567"))] + base[31:40]), FORMAT)
    add("faults nobody looks up", pairs_text([(first_line(o), b) for o, b in zip(others, ["....(-5.30)", plain_line("-1e2"), plain_line("- 5.3"),
                                                                                        plain_line("1234567890.123456"), "", "x"])] + base))
    add("a refused pair replaced by a later one", pairs_text([(first_line(guides[0]), "....(-5.30)")] + base))
    # sizes and the edges of the groups whose line ends one thread marks
    add("no text", b"")
    add("one byte", b"\n")
    add("one byte, no line end", b"G")
    add("one line", first_line(guides[0]).encode() + b"\n")
    a0, b0 = base[0]
    for name, end in (("CR LF across a group edge", "\r\n"), ("a lone CR as a group's last byte", "\r")):
        pad = (-(len(a0) + 1)) % group  # the first line's terminator starts at the group's last byte
        line = a0 + "x" * pad
        assert (len(line) + 1) % group == 0
        add(name, (line + end + b0 + end).encode() + pairs_text(base[1:10], end))
        add(name + ", behind the second line", pairs_text(base[1:2]) +
            (a0 + "\n" + b0 + " " * ((-(len(pairs_text(base[1:2])) + len(a0) + 1 + len(b0) + 1)) % group) + end).encode() + pairs_text(base[2:10], end))
    for k in list(range(16)) + list(range(group - 16, group)):  # the first line ends on byte k of a group
        pad = (k - len(a0)) % group
        line = a0 + "y" * pad
        assert len(line) % group == k
        add("a line end on byte %d of a group" % k, (line + "\n" + b0 + "\n").encode() + pairs_text(base[1:4]))
    add("a first line of 100 KB", (a0 + "z" * 100000 + "\n" + b0 + "\n").encode() + pairs_text(base[1:5]))
    add("a second line of 100 KB", pairs_text(base[1:5]) + (a0 + "\n" + scaffold_line("-41.25", lead="." * 100000) + "\n").encode())
    add("a second line of 100 KB without the scaffold", (a0 + "\n" + "(" * 50000 + ")" * 50000 + " (-41.50)").encode())
    return cases
