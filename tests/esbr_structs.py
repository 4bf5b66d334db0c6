"""The mirrors of include/xaac_esbr.h (libxaac_amd.abi) under the tests' names, and new streams' states (test infrastructure)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # for runs with only tests/ and tools/ on it
from libxaac_amd.abi import EsbrAnaState as EsbrAna, EsbrSynState as EsbrSyn  # noqa: E402,F401
from libxaac_amd.abi import EsbrPsState, EsbrPvcSide, EsbrPvcState, EsbrSide, EsbrState, PvcFrame, PvcState  # noqa: E402,F401


def new_state():
    st = EsbrState()
    st.esbr_start_up = 1
    return st


def new_ps_state():
    st = EsbrPsState()
    for j in range(20):
        st.h_prev[0][j] = 1.0
        st.h_prev[1][j] = 1.0
    return st
