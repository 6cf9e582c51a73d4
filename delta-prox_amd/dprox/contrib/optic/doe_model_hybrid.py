"""The reference's hybrid refractive / diffractive model is built as ``dprox.contrib.optic.doe_hybrid``; this module name still raises."""
raise NotImplementedError("dprox.contrib.optic.doe_model_hybrid is not importable on this backend: the hybrid model lives in "
                          "dprox.contrib.optic.doe_hybrid (same names and defaults: HeightMap, RGBCollimator, DOEModelConfig, "
                          "build_doe_model, build_baseline_profile, wvls, RI)")
