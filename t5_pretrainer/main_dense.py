from ripor_amd.main_dense import *  # noqa: F401,F403
from ripor_amd.main_dense import main

if __name__ == "__main__":
    main()
