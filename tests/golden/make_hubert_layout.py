"""Generate tests/golden/hubert_layout.json: the HuBERT backbone's packed-blob size, workspace size and every workspace member's
(offset, bytes) as the built library answers them (tests/hubert_audit_util.py: layout_records; no GPU).

The committed file was recorded from the library of the commit before NativeHubert's host side was merged into one
dtype-parameterised description; tests/test_hubert_audit_host.py holds every later library to it.  A
change that means to move a layout regenerates it and says so.

Run from the repository root: python tests/golden/make_hubert_layout.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "edge-diffusion-tts_amd"), os.path.join(REPO, "tests"), REPO]


def main():
    import hubert_audit_util as HU
    rec = HU.layout_records()
    with open(HU.LAYOUT_GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{HU.LAYOUT_GOLDEN}: {len(rec)} records")


if __name__ == "__main__":
    main()
