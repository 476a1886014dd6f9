"""Plain numpy / Python model of issl_consensus_begin and issl_consensus_finish as include/issl_hip.h specifies them: the
steps of Crackling.py:306-598 for one guide at a time, each behind the filter of :36-149.  Nothing of the library runs
here.  Codes: 0 rejected, 1 accepted, 2 untested ('?'), 3 error ('!')."""
import csv
import json
import pathlib

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "consensus"
NO, YES, UNTESTED, ERROR = 0, 1, 2, 3
CODES = "01?!"
LEVELS = {"ultralow": 0, "low": 1, "medium": 2, "high": 3}
CODE_FIELDS = ("g20", "lead_t", "at_pct", "tttt", "ss", "mm10db", "sgrna")
ROW_DTYPE = np.dtype([("sgrna_score", "<f8"), ("at", "<f8"), ("ss_energy", "<f8"), ("g20", "u1"), ("lead_t", "u1"),
                      ("at_pct", "u1"), ("tttt", "u1"), ("ss", "u1"), ("mm10db", "u1"), ("sgrna", "u1"), ("count", "u1")])
# the reference's column of every field of a row
COLUMNS = {"g20": "passedG20", "lead_t": "passedAvoidLeadingT", "at_pct": "passedATPercent", "tttt": "passedTTTT",
           "ss": "passedSecondaryStructure", "mm10db": "acceptedByMm10db", "sgrna": "acceptedBySgRnaScorer"}
# bit j of position p's four inputs: A 0001, C 0010, T 0100, G 1000 read as strings, index 0 first
ONEHOT = {"A": 3, "C": 2, "T": 1, "G": 0}


def onehot(guides):
    x = np.zeros((len(guides), 80), dtype=np.int64)
    for r, g in enumerate(guides):
        for p in range(20):
            x[r, 4 * p + ONEHOT[g[p]]] = 1
    return x


def sgrna_scores(guides, sv, coef, intercept):
    """-((((0.0 + coef[0] * k_0) + coef[1] * k_1) ...) + intercept), every product and sum a double of its own."""
    k = onehot(guides) @ np.asarray(sv, dtype=np.int64).T  # [n, n_sv], exact
    acc = np.zeros(len(guides), dtype=np.float64)
    for i in range(len(coef)):
        acc = acc + np.float64(coef[i]) * k[:, i].astype(np.float64)
    return -(acc + np.float64(intercept))


class Model:
    """begin in the constructor (-> .rows so far, .fold_rows), then finish(folds) (-> .rows, .selected)."""

    def __init__(self, guides, seen, optimisation="high", n=2, mm10db=True, chopchop=True, sgrnascorer2=True, model=None,
                 sgrna_threshold=0.0, low_energy=-30.0, high_energy=-18.0):
        self.guides = list(guides)
        self.unique = [int(s) == 1 for s in seen]
        self.level = LEVELS[optimisation] if isinstance(optimisation, str) else int(optimisation)
        self.n, self.mm10db, self.chopchop, self.sgrna = int(n), bool(mm10db), bool(chopchop), bool(sgrnascorer2)
        self.model, self.threshold, self.low, self.high = model, float(sgrna_threshold), float(low_energy), float(high_energy)
        rows = np.zeros(len(self.guides), dtype=ROW_DTYPE)
        for f in ("sgrna_score", "at", "ss_energy"):
            rows[f] = np.nan
        for f in CODE_FIELDS:
            rows[f] = UNTESTED
        self.rows = rows
        fold = []
        for j, g in enumerate(self.guides):
            r = rows[j]
            if self.chopchop and self.assess("chopchop", j):
                r["g20"] = YES if g[19] == "G" else NO
            if self.mm10db:
                if self.assess("mm10db", j):
                    r["lead_t"] = NO if g[0] == "T" else YES
                if self.assess("mm10db", j):
                    at = 100.0 * sum(c in "AT" for c in g[0:20]) / 20.0
                    r["at"] = at
                    r["at_pct"] = NO if at < 20 or at > 65 else YES
                if self.assess("mm10db", j):
                    r["tttt"] = NO if "TTTT" in g else YES
                if self.assess("mm10db", j):
                    fold.append(j)
        self.fold_rows = np.array(fold, dtype=np.uint32)
        self.selected = None

    def assess(self, module, j):
        r = self.rows[j]
        if self.level == 0:
            return True
        if not self.unique[j]:
            return False
        if self.level == 1:
            return True
        if module == "specificity":
            return int(r["count"]) >= self.n
        if self.level == 3:
            verdicts = (r["mm10db"], r["g20"], r["sgrna"])
            accepted = sum(v == YES for v in verdicts)
            assessed = sum(v in (YES, NO) for v in verdicts)
            tools = self.mm10db + self.chopchop + self.sgrna
            if accepted >= self.n:
                return False
            if tools - assessed < self.n - accepted:
                return False
        if module == "mm10db" and NO in (r["lead_t"], r["at_pct"], r["tttt"], r["ss"], r["mm10db"]):
            return False
        return True

    def finish(self, folds=None):
        assert self.selected is None, "finish is called once"
        n_folds = 0 if folds is None else len(folds)
        assert n_folds == len(self.fold_rows)
        rows = self.rows
        for i, j in enumerate(self.fold_rows):
            f = folds[i]
            if not f["present"]:
                continue
            rows[j]["ss_energy"] = f["energy"]
            if self.guides[j][0] == "T":
                rows[j]["ss"] = ERROR
            elif f["scaffold"]:
                rows[j]["ss"] = NO if f["energy"] < self.low else YES
            else:
                rows[j]["ss"] = NO if f["energy"] <= self.high else YES
        scores = sgrna_scores(self.guides, *self.model) if self.sgrna else None
        selected = []
        for j in range(len(self.guides)):
            r = rows[j]
            if self.mm10db:
                r["mm10db"] = YES if all(r[f] == YES for f in ("at_pct", "tttt", "ss", "lead_t")) else NO
            if self.sgrna and self.assess("sgrnascorer2", j):
                r["sgrna_score"] = scores[j]
                r["sgrna"] = NO if scores[j] < self.threshold else YES
            r["count"] = int(r["mm10db"] == YES) + int(r["sgrna"] == YES) + int(r["g20"] == YES)
            if self.assess("specificity", j):
                selected.append(j)
        self.selected = np.array(selected, dtype=np.uint32)
        return self


# ---- the goldens ------------------------------------------------------------------------------------------------------

def golden_configs():
    """-> [{"name", "optimisation", "n", "mm10db", "chopchop", "sgrnascorer2", thresholds}] of tests/golden/consensus."""
    return json.loads((GOLDEN / "configs.json").read_text())


def golden_keywords(cfg):
    sv, coef, intercept = golden_model()
    return dict(optimisation=cfg["optimisation"], n=cfg["n"], mm10db=cfg["mm10db"], chopchop=cfg["chopchop"],
                sgrnascorer2=cfg["sgrnascorer2"], model=(sv, coef, intercept), sgrna_threshold=cfg["sgrna_threshold"],
                low_energy=cfg["low_energy"], high_energy=cfg["high_energy"])


def golden_model():
    z = np.load(GOLDEN / "model.npz")
    return z["sv"], z["coef"], float(z["intercept"])


def golden_rows(name):
    with open(GOLDEN / f"{name}.csv", newline="") as fh:
        return list(csv.DictReader(fh))


def fold_text():
    return (GOLDEN / "fold.txt").read_text()


def fold_energies(text):
    """guide[1:20] -> the energy of its last pair in RNAfold's output, for the rows whose ssEnergy the reference cuts
    out with a split at blanks (Crackling.py:470), which leaves nothing of a padded "( -5.30)"."""
    lines = text.splitlines()
    out = {}
    for a, b in zip(lines[0::2], lines[1::2]):
        out[a[1:20].replace("U", "T")] = float(b[b.rindex("(") + 1:b.rindex(")")])
    return out


def compare_with_reference(rows, guides, seen, want, energies):
    """rows (ROW_DTYPE-like structured array) against the reference's own output rows `want` for the same guides."""
    assert len(rows) == len(want)
    for j, (r, w) in enumerate(zip(rows, want)):
        what = f"row {j} {w['seq']}"
        assert guides[j] == w["seq"], what
        assert ("1" if seen[j] == 1 else "0") == w["isUnique"], what
        for f, col in COLUMNS.items():
            assert CODES[r[f]] == w[col], f"{what}: {col} {CODES[r[f]]} != {w[col]}"
        assert str(int(r["count"])) == w["consensusCount"], f"{what}: consensusCount {r['count']} != {w['consensusCount']}"
        for f, col in (("sgrna_score", "sgrnascorer2score"), ("at", "AT")):
            if w[col] == "?":
                assert np.isnan(r[f]), f"{what}: {col}"
            else:  # shortest round-trip digits: equal strings mean equal doubles and the other way round
                assert float(w[col]) == r[f], f"{what}: {col} {r[f]!r} != {w[col]}"
        if w["ssEnergy"] == "?":
            assert np.isnan(r["ss_energy"]), f"{what}: ssEnergy"
        elif w["ssEnergy"] == "":  # a padded energy: the reference's split keeps nothing, its verdict uses the number
            assert r["ss_energy"] == energies[guides[j][1:20]], f"{what}: ssEnergy of a padded line"
        else:
            assert float(w["ssEnergy"]) == r["ss_energy"], f"{what}: ssEnergy {r['ss_energy']!r} != {w['ssEnergy']}"
