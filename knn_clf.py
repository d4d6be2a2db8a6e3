"""Entry point: `python knn_clf.py ...`, weighted k-nearest-neighbour accuracy of pretraining checkpoints on their frozen image features, with
voc_clf.py's command line plus --k and --temperature (clip-lite_amd/downstream.py, clip-lite_amd/knn.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clip_lite_amd.downstream import knn_clf_cli  # noqa: E402

if __name__ == "__main__":
    knn_clf_cli()
