"""CPU: the training step's Python wiring is four modules (train_state < train_perop < train_fusedfn < train_ops).  What the
rest of the repository reaches through `train_ops` still resolves there, shared state is ONE object behind both names, the
switches assigned on `train_ops` are the ones its functions read, and the inference path of the continuous model does not load
the training step."""
import os
import subprocess
import sys

import torch

from puflow_amd import train_fusedfn, train_ops, train_perop, train_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every name that tests/, tools/ and the package's other modules reach as train_ops.NAME or import from it
NAMES = """
_FUSED _FOLD_WU _CHAIN _GLUE _PERSIST _PREFOLD _TAP _FANOUT
forward_train edgeconv_train edgeconv_train_fused ec_prefold cond_net_fused
set_deterministic deterministic sync_bn check_persist_status
_SYNCW _STAT _DW_STREAMS _FC_IMG _sync_words _sync_cb_impl _attach_sync _zeros_kept _multi_rank _dw_begin _stream _side_stream
_gemm linear bn_lrelu cond_net _mlp_bn knn_csr knn_csr_pair mlp_fused bnmlp_fused
ActFn BnLreluFn EdgeFeatureFn GatherRowsFn MaxPoolKFn RepeatRowsFn SoftmaxWsumFn
InterpWsumFn FoldWuFn ParamFanFn EdgeConvUnitFn FlowChainFn MlpFn CondNetStackFn CondNetBatchFn MergeBatchFn BnMlpFn FanoutFn
""".split()

SWITCHES = ("_FUSED", "_FOLD_WU", "_CHAIN", "_GLUE", "_PERSIST", "_PREFOLD", "_TAP", "_FANOUT")


def test_names_reached_through_train_ops_resolve():
    missing = [n for n in NAMES if not hasattr(train_ops, n)]
    assert not missing, f"no longer on puflow_amd.train_ops: {missing}"


def test_shared_state_is_one_object_behind_both_names():
    for name in ("_SYNCW", "_STAT", "_DW_STREAMS", "_FC_IMG"):
        assert getattr(train_ops, name) is getattr(train_state, name), name


def test_no_switch_lives_outside_train_ops():
    for mod in (train_state, train_perop, train_fusedfn):
        assert not [s for s in SWITCHES if hasattr(mod, s)], mod.__name__


def test_switches_assigned_on_train_ops_are_the_ones_read():
    units, x0 = [object()], torch.zeros(1, 16, 3)
    was = train_ops._FUSED, train_ops._PREFOLD
    try:
        try:
            train_ops.ec_prefold(units, x0, 16)
            raise AssertionError("with the defaults ec_prefold passes its switches and reaches p.convs")
        except AttributeError:
            pass
        train_ops._FUSED = False
        assert train_ops.ec_prefold(units, x0, 16) is None
        train_ops._FUSED = was[0]
        train_ops._PREFOLD = False
        assert train_ops.ec_prefold(units, x0, 16) is None
    finally:
        train_ops._FUSED, train_ops._PREFOLD = was


def test_deterministic_flag_is_one_flag():
    was = train_state.deterministic()
    try:
        for on in (True, False):
            train_ops.set_deterministic(on)
            assert train_ops.deterministic() is on and train_state.deterministic() is on
    finally:
        train_state.set_deterministic(was)


def test_cnf_inference_does_not_load_the_training_step():
    code = "import sys, puflow_amd.cnf; sys.exit(int('puflow_amd.train_ops' in sys.modules))"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
