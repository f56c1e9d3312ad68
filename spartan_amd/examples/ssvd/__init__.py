"""The first step of the reference's stochastic SVD family (spartan/examples/ssvd): the thin Cholesky-QR."""
