"""Drop-in entry point: `python voc_clf.py ...` with the reference's command line (reference voc_clf.py): VOC2007 linear-SVM mAP of pretraining
checkpoints, with the batched GPU SVM solver of clip_lite_amd (clip-lite_amd/downstream.py, clip-lite_amd/svm.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clip_lite_amd.downstream import voc_clf_cli  # noqa: E402

if __name__ == "__main__":
    voc_clf_cli()
