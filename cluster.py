"""Drop-in entry point: `python cluster.py ...` with the reference's command line (reference scripts/cluster.py): caption embeddings of the
pretraining dataset, k-means on the GPU for every cluster count, and the img_id_*_map pickles that DATA.CLUSTER_PATH points at for clustered
negative sampling (clip-lite_amd/downstream.py, clip-lite_amd/kmeans.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from clip_lite_amd.downstream import cluster_cli  # noqa: E402

if __name__ == "__main__":
    cluster_cli()
