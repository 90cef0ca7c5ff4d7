# make_golden_diffmap.jl -- UNEXECUTED in this repository (Julia is absent from its images).
#
# method = :diffusion is pinned to diffmap.py, and that is pinned to nothing: it restates ManifoldLearning 0.6.2's DiffMap from
# memory.  A maintainer with Julia 1.5 and the reference's Manifest.toml pins (ManifoldLearning 0.6.2, Project.toml:47) runs this
# once; it reads the committed snapshot stream, forms the deviation matrix as src/subspace_construction.jl:181-200 does and writes
# what the REAL package computes for it:
#
#     julia --project=/path/to/SubspaceInference.jl tests/golden/make_golden_diffmap.jl
#
# diffmap_reference.npz then holds A (N x K), P (N x M, the reference's `P'` of :206), the kernel matrix and the eigenvalues the
# model kept.  Compare with diffmap.diffmap_dense(A, M, eps, alpha, kernel_sign, rescale): the four keywords are the points where
# memory may be wrong (the sign in the exponent above all), and whichever setting reproduces P up to column signs becomes the
# default of si_construct_finish_diffmap's callers -- no kernel changes.
using ManifoldLearning, LinearAlgebra
using NPZ   # ] add NPZ

here = @__DIR__
toy = npzread(joinpath(here, "toy_construct_k12.npz"))
snaps, ns = toy["snapshots"], toy["ns"]                 # K x N Float32, K
N = size(snaps, 2)
W_swa = zeros(N)                                        # :174
A = Float64[]
for k in 1:size(snaps, 1)
    W = snaps[k, :]
    n = ns[k]
    global W_swa = (n .* W_swa + W) ./ (n + 1)          # :188
    W_dev = W - W_swa                                   # :192
    append!(A, W_dev)                                   # :193
end
A = reshape(A, N, :)                                    # :202
M = 3
diff_M = fit(DiffMap, A', maxoutdim = M)                # :204
P = transform(diff_M)                                   # :205   (M x N)
npzwrite(joinpath(here, "diffmap_reference.npz"),
         Dict("W_swa" => W_swa, "A" => A, "P" => Matrix(P'), "kernel" => Matrix(ManifoldLearning.kernel(diff_M)),
              "lambda" => diff_M.λ, "M" => M))
