"""Constants the hot-path operators read (reference: src/pydrobert/torch/config.py)."""

import math

INDEX_PAD_VALUE = -100  # config.py:55
DEFT_INS_COST = 1.0  # config.py:156
DEFT_DEL_COST = 1.0  # config.py:159
DEFT_SUB_COST = 1.0  # config.py:162
DEFT_PAD_VALUE = 0.0
TINY = 1.1754943508222875e-38  # config.py: the smallest normal float32
EPS_NINF = math.log(1.1754943508222875e-38) / 2  # config.py:79: log of the smallest normal float32, halved
EPS_0 = math.log1p(-2 * 1.1920928955078125e-07)  # config.py:86
EPS_INF = math.log(3.4028234663852886e38) / 2  # config.py:93: log of the largest float32, halved
