"""Drop-in entry point: `python retrieval.py ...` with the reference's command line (reference retrieval.py): image-text retrieval recall@1/5/10
of a pretraining checkpoint on COCO / Flickr30k, with the ranking on the GPU (clip-lite_amd/downstream.py, clip-lite_amd/retrieval.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clip_lite_amd.downstream import retrieval_cli  # noqa: E402

if __name__ == "__main__":
    retrieval_cli()
