"""Records tests/golden/wgrad_bits.json: SHA-256 of dw after every case of tests/test_wgrad_bits_gpu.py, on the MI355X, at the
commit whose launches the test pins -- 1ee94b0 ("Pin the operand-prep kernels bit for bit; NaN and inf survive a conv"), the parent
of the change that gave the weight gradient's routing one owner.

    (check out 1ee94b0 next to this file and tests/test_wgrad_bits_gpu.py, build the library)
    python tests/golden/gen_golden_wgrad_bits.py [output path]

Every case runs twice; a case whose two digests differ is not repeatable and is refused (the file is not written)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "mmt-psm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_wgrad_bits_gpu as T  # noqa: E402


def main():
    from maskrcnn_benchmark import _hip as H
    H.lib()
    out, bad = {}, []
    runs = [(name, lambda n=name: T.run_case(H, n)) for name in sorted(T.CASES)] + [("group_of_two", lambda: T.run_group(H))]
    for name, run in runs:
        a, b = run(), run()
        print(name, a, "repeatable" if a == b else "NOT REPEATABLE: " + b, flush=True)
        if a != b:
            bad.append(name)
        out[name] = a
    if bad:
        raise SystemExit("not repeatable at this commit: %s" % ", ".join(bad))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wgrad_bits.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
