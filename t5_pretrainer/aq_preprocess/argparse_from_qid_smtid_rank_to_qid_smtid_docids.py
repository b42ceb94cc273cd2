from ripor_amd.aq_preprocess.argparse_from_qid_smtid_rank_to_qid_smtid_docids import main

if __name__ == "__main__":
    main()
