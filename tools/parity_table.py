#!/usr/bin/env python3
"""Per-tensor worst parity figures of a suite run, as a markdown table.

Input: the record files of the tools/parity_record.py pytest plugin (a line
per close(..., mag=M) comparison: test id, tensor, label, pass/FAIL, element
count, normwise error, max relative error above the 1e-2 floor, max absolute
error per max|ref| below it, p50 / p99 / p100 relative error).

    PYTHONPATH=tools DDQ_PARITY_FIGURES=figures.tsv pytest -p parity_record -m gpu
    tools/parity_table.py figures.tsv [more.tsv ...]

Each figure's maximum is given with the test (and label) that produced it.
Comparisons the suite expects to fail (the mutation tests) are left out; any
other FAIL record is listed below the table.
"""
import collections
import sys

ORDER = ["Q_out", "P_out", "Qn_out", "Q_sa", "P_sa", "target_Q_sa", "Q_out.diff", "loss",
         "Qconv1[0]", "Qconv1[1]", "Qconv2[0]", "Qconv2[1]", "Qconv3[0]", "Qconv3[1]",
         "Qfc4[0]", "Qfc4[1]", "Q_out[0]", "Q_out[1]"]
BOUNDS = (1e-5, 1e-4, 1e-6)


def short(test):
    return test.split("::", 1)[-1] if "::" in test else test


def main(paths):
    worst = collections.defaultdict(lambda: [(0.0, "-")] * 3)
    count = collections.Counter()
    fails = []
    for p in paths:
        for line in open(p):
            f = line.rstrip("\n").split("\t")
            if len(f) != 11:
                continue
            test, key, what, status = f[0], f[1], f[2], f[3]
            if "rejects_mutated" in test:
                continue
            if status != "pass":
                fails.append(line.rstrip("\n"))
                continue
            count[key] += 1
            figs = [float(v) for v in f[5:8]]
            label = short(test) + (" (%s)" % what if what != key else "")
            worst[key] = [max(a, (v, label)) for a, v in zip(worst[key], figs)]
    keys = [k for k in ORDER if k in worst] + sorted(k for k in worst if k not in ORDER)
    print("| tensor | comparisons | normwise (≤ 1e-5) | rel above 1e-2·max (≤ 1e-4) | "
          "abs below, per max (≤ 1e-6) |")
    print("|---|---|---|---|---|")
    for k in keys:
        cells = ["%.2e — %s" % (v, lab) if v > 0 else "0" for v, lab in worst[k]]
        print("| %s | %d | %s |" % (k, count[k], " | ".join(cells)))
    print()
    for i, name in enumerate(("normwise", "rel above the floor", "abs below the floor")):
        v, k = max((worst[k][i][0], k) for k in keys)
        print("worst %s: %.3g (%s), %.1fx inside %g" % (name, v, k, BOUNDS[i] / v if v else 0,
                                                       BOUNDS[i]))
    if fails:
        print("\nFAIL records:")
        for ln in fails:
            print(ln)


if __name__ == "__main__":
    main(sys.argv[1:])
