"""Build-authored, test-only stand-in for the `tensorflow_probability` names the reference's optimizer_cem_gmm_tf.py touches
(see README.md beside this file); torch-CPU fp32 tensors like standins/tensorflow."""
