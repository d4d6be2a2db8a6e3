"""Entry point: `python logreg_clf.py ...`, the logistic-regression probe of pretraining checkpoints on their frozen image features, with
knn_clf.py's command line plus --cost, --holdout and --tol (clip-lite_amd/downstream.py, clip-lite_amd/logreg.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clip_lite_amd.downstream import logreg_clf_cli  # noqa: E402

if __name__ == "__main__":
    logreg_clf_cli()
