"""Entry point: `python bias_eval.py ...`, the bias evaluation of a pretraining checkpoint: a direction found in the text embeddings of
definitional word pairs is removed from the image features, and what each prompt retrieves from every group of images is compared before and
after (clip-lite_amd/downstream.py, clip-lite_amd/debias.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clip_lite_amd.downstream import bias_eval_cli  # noqa: E402

if __name__ == "__main__":
    bias_eval_cli()
