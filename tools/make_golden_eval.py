"""Records tests/golden/palette_mfnet.json: the nine class colours the upstream reference renders label maps with
(util/util.py:8-19, get_palette()).  Generator only - needs a checkout of the reference, which the tests do not:

    python tools/make_golden_eval.py --reference DIR

The reference's file imports PIL at its top and does not use it in get_palette(); an empty stand-in module serves when PIL
is absent.  The fixture is 27 numbers and the class names, no program text.
"""
import argparse
import importlib.util
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["unlabeled", "car", "person", "bike", "curve", "car_stop", "guardrail", "color_cone", "bump"]  # util/util.py:7


def load_reference_util(ref_root):
    path = os.path.join(ref_root, "util", "util.py")
    if not os.path.isfile(path):
        raise RuntimeError(f"{path} not found: pass the reference checkout with --reference")
    try:
        import PIL  # noqa: F401
    except ImportError:
        pil = types.ModuleType("PIL")
        pil.Image = types.ModuleType("PIL.Image")
        sys.modules["PIL"], sys.modules["PIL.Image"] = pil, pil.Image
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("_segmif_ref_util", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "palette_mfnet.json"))
    args = ap.parse_args()
    palette = load_reference_util(args.reference).get_palette()
    assert palette.shape == (len(NAMES), 3) and palette.min() >= 0 and palette.max() <= 255
    with open(args.out, "w") as f:
        json.dump({"source": "util/util.py:8-19 get_palette()", "names": NAMES, "palette": palette.tolist()}, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
