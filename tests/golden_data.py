"""Stored test vectors under tests/golden/.

``fewrel_val.json.xz``: the FewRel 1.0 validation file (16 relations x 700 instances, the ``val.json`` the
reference trains and validates on), xz-compressed to stay below the repository's file size limit.
"""
import lzma
import os
import shutil

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fewrel_val_json(dest_dir) -> str:
    """Unpack the stored FewRel validation file into ``dest_dir`` and return the path of ``val.json``."""
    out = os.path.join(str(dest_dir), "val.json")
    if not os.path.exists(out):
        with lzma.open(os.path.join(GOLDEN, "fewrel_val.json.xz"), "rb") as src, open(out, "wb") as dst:
            shutil.copyfileobj(src, dst)
    return out
