"""Drop-in name for maua/audiovisual/audioreactive/selfsupervised/features/correlation.py: re-exports the MI355X-native implementation in maua_amd."""
from maua_amd.correlation import (_coxhead, _coxhead2, _rvadj_ghaziri, _rvadj_maye, autocorrcorr, concordance, lcka, op, pearson,  # noqa: F401
                                  pwcca, r1, r3, rv, rv2, smi, spearman, svcca)
