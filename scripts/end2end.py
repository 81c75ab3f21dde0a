"""Drop-in for the reference's scripts/end2end.py on the HIP retriever and reader (multihop_dense_retrieval_amd/end2end.py has the
flags and the deliberate differences).

    python scripts/end2end.py hotpot_qas_val.json --indexpath wiki_index.npy --corpus_dict hotpotQA_corpus_dict.json \
        --retriever_path q_encoder.pt --reader_path qa_electra.pt --topk 20 --batch-size 100 --sp-pred --save-prediction out.json
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

if __name__ == "__main__":
    from multihop_dense_retrieval_amd import end2end
    end2end.main()
