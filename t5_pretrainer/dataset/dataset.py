from ripor_amd.dataset.lng_knp import *  # noqa: F401,F403
from ripor_amd.dataset.seq2seq import Seq2SeqForT5SeqAQDataset  # noqa: F401
from ripor_amd.dataset.pretrain import MarginMSEforPretrainDataset  # noqa: F401
from ripor_amd.dataset.margin_mse import MarginMSEforT5SeqAQDataset  # noqa: F401
