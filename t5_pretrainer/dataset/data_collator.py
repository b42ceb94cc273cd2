from ripor_amd.dataset.lng_knp import LngKnpMarginMSEforT5SeqAQCollator  # noqa: F401
from ripor_amd.dataset.seq2seq import Seq2SeqForT5SeqAQCollator  # noqa: F401
from ripor_amd.dataset.pretrain import MarginMSEforPretrainCollator  # noqa: F401
from ripor_amd.dataset.margin_mse import MarginMSEforT5SeqAQCollator  # noqa: F401
