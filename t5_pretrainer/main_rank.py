from ripor_amd.main_rank import *  # noqa: F401,F403
from ripor_amd.main_rank import main

if __name__ == "__main__":
    main()
