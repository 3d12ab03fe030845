"""``LSTMWakeword`` with the constructor, ``forward`` contract and ``state_dict`` keys of the reference class
(``src/models/architectures.py``: ``lstm.weight_ih_l0`` ... ``lstm.bias_hh_l1_reverse``, ``fc.1.weight``, ``fc.1.bias``), running on
``ww_lstm_*`` (one persistent MFMA kernel per layer for both directions), ``ww_dropout_bt`` and the MFMA ``fc``.  Like
``GRUWakeword`` it also accepts the (B,1,F,T) feature batches the Trainer produces.  Hidden size 128 (the reference default) is
the implemented size; dropout masks come from the GRU's Philox streams (inter-layer ``1 + k``, head 15).  The layer stack and
the head are the GRU's (recurrent.py)."""
from .. import _native as nat
from .flat_buckets import FlatBuckets
from .recurrent import _NativeRNN, _RNNWakewordBase


class NativeLSTM(_NativeRNN):
    """nn.LSTM's parameters on ww_lstm_*; a bidirectional layer is always ONE launch, eager and under graph capture alike."""
    cell = nat._LSTM
    overlap_directions = False


class LSTMWakeword(FlatBuckets, _RNNWakewordBase):
    """The reference's LSTMWakeword.  Its parameters live in one flat bucket (fused clip + optimizer, one all-reduce,
    graph-capturable step)."""
    stack, stack_name = NativeLSTM, "lstm"
