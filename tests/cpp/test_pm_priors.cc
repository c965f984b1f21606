// Drives the ProbabilityMapping class with sdm::Options::device_priors on or off (argv[4] = 1 / 0) over one sequence of
// keyframes that carry ORB observations (map point ids, keypoint angles, point depths): SemiDenseRecon per keyframe in
// map order (argv[5] = "recon"), or one SemiDenseReconBlock over the whole map (argv[5] = "block").  Writes every
// keyframe's flags and maps to argv[2] and the point cloud to argv[3]; tests/test_gpu_cpp_priors.py runs it both ways and
// compares the bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sdm/ProbabilityMapping.h"

static void rd(FILE* f, void* p, size_t n)
{
    if (n && fread(p, 1, n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
}

template <typename T>
static void rd_vec(FILE* f, std::vector<T>& v)
{
    int n;
    rd(f, &n, sizeof(int));
    v.resize(n);
    rd(f, v.data(), sizeof(T) * n);
}

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[4];
    rd(f, hdr, sizeof(hdr));
    const int W = hdr[0], H = hdr[1], n_kf = hdr[2], covisN = hdr[3];
    std::vector<sdm::KeyFrame> kfs(n_kf);
    std::vector<std::vector<int>> covis(n_kf);
    for (int k = 0; k < n_kf; k++) {
        sdm::KeyFrame& kf = kfs[k];
        kf.mnId = k;
        kf.im_ = sdm::Mat<uint8_t>(H, W);
        rd(f, kf.im_.ptr(), (size_t)W * H);
        float K[4];
        rd(f, K, sizeof(K));
        kf.fx = K[0];
        kf.fy = K[1];
        kf.cx = K[2];
        kf.cy = K[3];
        rd(f, kf.Tcw, sizeof(float) * 12);
        rd_vec(f, covis[k]);
        rd_vec(f, kf.point_depths);
        rd_vec(f, kf.map_point_ids);
        rd_vec(f, kf.keypoint_angles);
    }
    fclose(f);
    sdm::Map map;
    for (int k = 0; k < n_kf; k++) {
        for (int j : covis[k]) kfs[k].covisible.push_back(&kfs[j]);
        map.keyframes.push_back(&kfs[k]);
    }
    sdm::Options opt;
    opt.covisN = covisN;
    opt.max_keyframes = n_kf;
    opt.device_priors = atoi(argv[4]) != 0;
    ProbabilityMapping pm(&map, opt);
    if (std::string(argv[5]) == "block") {
        pm.SemiDenseReconBlock(map.keyframes, 0, n_kf);
    } else {
        for (int k = 0; k < n_kf; k++) pm.SemiDenseRecon(&kfs[k]);
    }
    if (!pm.ok()) return 3;
    long nv = pm.SavePointCloudObj(argv[3]);

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (int k = 0; k < n_kf; k++) {
        int flags[2] = {kfs[k].semidense_flag_, kfs[k].interKF_depth_flag_};
        fwrite(flags, sizeof(int), 2, o);
        fwrite(kfs[k].depth_map_.ptr(), sizeof(float), (size_t)W * H, o);
        fwrite(kfs[k].depth_sigma_.ptr(), sizeof(float), (size_t)W * H, o);
        fwrite(kfs[k].SemiDensePointSets_.ptr(), sizeof(float), (size_t)3 * W * H, o);
    }
    fwrite(&nv, sizeof(long), 1, o);
    fclose(o);
    return 0;
}
