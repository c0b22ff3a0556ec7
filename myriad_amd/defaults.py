"""Per-system extragradient step sizes (/root/reference/myriad/defaults.py:5-18) and the start values of the parameter fits
(:20-91; experiments/mle_sysid.py starts from them and fits exactly these keys)."""
from myriad_amd.systems import SystemType

learning_rates = {
  SystemType.CANCERTREATMENT: {'eta_x': 1e-1, 'eta_v': 1e-3},
  SystemType.CARTPOLE: {'eta_x': 1e-2, 'eta_v': 1e-4},
}

_T = SystemType
param_guesses = {                                           # defaults.py:20-91 (true values: the systems' constructor defaults)
  _T.BACTERIA: {'r': 0.8, 'A': 1.2, 'B': 2.},
  _T.BEARPOPULATIONS: {'r': .2, 'K': .6, 'm_f': .3, 'm_p': .6},
  _T.BIOREACTOR: {'D': 0.8, 'G': 1.2},
  _T.PENDULUM: {'g': 15., 'm': 3., 'length': 0.5},
  _T.CARTPOLE: {'g': 10., 'm1': 1.5, 'm2': 0.2, 'length': 0.6},
  _T.CANCERTREATMENT: {'r': 0.1, 'delta': 0.8},             # `a` enters the cost only: not fitted
  _T.GLUCOSE: {'a': 0.5, 'b': 0.4, 'c': 0.6},
  _T.HIVTREATMENT: {'k': .000044, 'm_1': .01, 'm_2': .9, 'm_3': 3.4, 'N': 250., 'r': 0.02, 's': 11., 'T_max': 1400.},
  _T.MOULDFUNGICIDE: {'r': 0.1, 'M': 8.},
  _T.MOUNTAINCAR: {'power': 0.001, 'gravity': 0.005},
  _T.PREDATORPREY: {'d_1': 0.15, 'd_2': 0.07},
  _T.TIMBERHARVEST: {'k': 0.7},
  _T.TUMOUR: {'xi': 0.06, 'b': 4.5, 'd': 0.01, 'G': 0.2, 'mu': 0.01},
  _T.VANDERPOL: {'a': 0.5},
}
