"""Drop-in entry point: `python zero_shot.py ...` with the reference's command line (reference zero_shot.py), running the MI355X-native downstream
evaluation of clip_lite_amd (clip-lite_amd/downstream.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clip_lite_amd.downstream import zero_shot_cli  # noqa: E402

if __name__ == "__main__":
    zero_shot_cli()
