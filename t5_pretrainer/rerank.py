from ripor_amd.rerank import *  # noqa: F401,F403
from ripor_amd.rerank import main

if __name__ == "__main__":
    main()
