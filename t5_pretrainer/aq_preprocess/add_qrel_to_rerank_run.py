"""alias package, see t5_pretrainer/__init__.py"""
import os
import sys

if __package__ in (None, ""):   # run by file path, as the reference's scripts do
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from ripor_amd.aq_preprocess.add_qrel_to_rerank_run import main  # noqa: E402

if __name__ == "__main__":
    main()
