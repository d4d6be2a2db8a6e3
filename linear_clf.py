"""Drop-in entry point: `python linear_clf.py ...` with the reference's command line (reference linear_clf.py), running the MI355X-native downstream
evaluation of clip_lite_amd (clip-lite_amd/downstream.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clip_lite_amd.downstream import linear_clf_cli  # noqa: E402

if __name__ == "__main__":
    linear_clf_cli()
