"""Generate tests/golden/sem_train_layout.json: the byte counts of the semantic head's training blob, tape and scratch, and code and
text of every refusal of its training entry points, as the built library answers them (tests/sem_layout_util.py: records; no GPU).

The committed file was recorded from the library of the commit before the host side of the FSQ and the VQ head was merged into
one description; tests/test_sem_layout_host.py holds every later library to it.  That library has no
edtts_sem_train_region, so the export is left out of the binding table when the loaded library lacks it.  A change that means to
move a layout or to reword a refusal regenerates the file and says so.

Run from the repository root: python tests/golden/make_sem_train_layout.py   (EDTTS_LIB=<path> records from another build)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "edge-diffusion-tts_amd"), os.path.join(REPO, "tests"), REPO]


def main():
    import ctypes
    from edge_diffusion_tts_amd import native
    if not hasattr(ctypes.CDLL(native.LIB_PATH), "edtts_sem_train_region"):  # a build from before the export
        native._ABI.pop("edtts_sem_train_region")
    import sem_layout_util as LU
    rec = LU.records()
    with open(LU.GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{LU.GOLDEN}: {len(rec['layouts'])} layouts, {len(rec['refusals'])} refusals")


if __name__ == "__main__":
    main()
