"""Workload drivers for the two application configs of BASELINE.json: `lreg` (configs[4], least squares
by gradient steps) and `sklearn.cluster.KMeans` (configs[3]); `logreg` is the logistic member of lreg's SGD family.
They are thin driver loops over the expression API; every per-tile body runs in HIP kernels through the backend.
`cholesky` (the blocked factorisation over map2's region join) and `ssvd.qr` (the thin Cholesky-QR) stand on the dense
factorisation kernels outside the tile path (sp_potrf / sp_trsm_rlt); `ssvd.ssvd` (the stochastic SVD: qr, then the
symmetric eigenproblem of the small B . B^T on sp_syevj) and `pca` (PCA on that SVD) complete the chain;
`sklearn.neighbors.NearestNeighbors` searches row bands of X with sp_knn and merges their candidates with sp_knn_merge;
`sklearn.manifold.Isomap` turns its lists into a graph (sp_graph_from_knn), takes all-pairs shortest paths (sp_apsp) and
embeds with sp_syevj; `als` (alternating least squares) solves every row's normal equations of a half-step in sp_als_solve;
`fuzzy_kmeans` runs one sp_fuzzy_step (memberships, labels and weighted sums fused) per row tile and iteration;
`lda.learn_topics` (LDA by collapsed variational Bayes) runs one sp_lda_step (the per-document loops fused) per tile of
documents and pass; `spectral_clustering.spectral_cluster` finds the degrees with one sp_affinity_degree and writes the
normalised affinity matrix with one sp_affinity_matrix per row band of the points (the affinity matrix itself is never
stored), and `lanczos.solve` (float64 on the host around `dot`) hands its leading Ritz vectors to KMeans;
`naive_bayes.fit` (the tf-idf naive Bayes classifier) runs one sp_nb_step (normalisation, label sums and document
frequencies fused) per row band of the documents, `predict` / `predict_labels` score with `dot` and `argmax`;
`nbody.move` / `simulate` (all-pairs gravity) runs one sp_nbody_accel (every pair in registers, nothing of size n x n)
per band of bodies and updates velocities and positions on the map kernels;
`cf.ItemBasedRecommender` (item-based collaborative filtering) runs one sp_item_topk (cosine similarity and top-k fused,
nothing of size N x N) per column band and source step of the rating table and merges the steps with sp_item_topk_merge;
`disdca_svm.fit` / `predict` (the linear SVM by distributed dual coordinate ascent) runs one sp_svm_dca (a band's whole
loop over its rows, w on chip) per row band and iteration and forms w with the reference's expression on the map and
reduce kernels;
`netflix.sgd` (stochastic-gradient matrix factorisation of a sparse rating matrix) runs one sp_sgd_mf (a block's
sequential loop over its ratings, level-scheduled, with the loop's bits) per block of a stratum and updates the factors
in place through select / update_slice;
`swaption.simulate` (European payer swaptions under the LIBOR market model by Monte Carlo) runs one sp_lmm_swaption (all
time steps of a band's antithetic pairs of paths, the forward rates on chip) per column band of a product's draws and
forms mean and standard error with the reference's expressions on the map and reduce kernels;
`canopy_clustering.canopy_cluster` / `find_centers` (canopy clustering) runs one sp_canopy (a tile's whole greedy loop
over its rows and its growing list of canopies, with the loop's bytes) per row tile and once more over the tiles'
centres, and labels every row tile with one sp_pdf_label in a lazy shuffle.
Like `sort` they are imported on first use, not with the package."""
