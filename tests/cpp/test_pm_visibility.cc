// Drives ProbabilityMapping::AppendTranscriptEntryWithVisibility (include/sdm/ProbabilityMapping.h): the class over the
// whole sequence in the reference's driver order (SemiDenseRecon per keyframe, PM.cc:137-315), then one transcript entry
// in the visibility-list form per keyframe.  tests/test_gpu_cpp_visibility.py writes the input blob (test_gpu_cpp_class.py's
// layout), repeats the call order on an Engine and compares the text.
//   argv: in.bin transcript.txt returns.txt
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <vector>

#include "sdm/ProbabilityMapping.h"

static void rd(FILE* f, void* p, size_t n)
{
    if (fread(p, 1, n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
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
        int nc;
        rd(f, &nc, sizeof(int));
        covis[k].resize(nc);
        rd(f, covis[k].data(), sizeof(int) * nc);
        int nd;
        rd(f, &nd, sizeof(int));
        kf.point_depths.resize(nd);
        rd(f, kf.point_depths.data(), sizeof(float) * nd);
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
    ProbabilityMapping pm(&map, opt);
    // the neighbours PM.cc:151-160 picks (every keyframe here is good and mapped: the first covisN covisible ones);
    // camera index of keyframe k in the transcript: 100 + k
    auto row = [&](int k, std::vector<sdm::KeyFrame*>& nb, std::vector<int>& cam) {
        nb.clear();
        cam.clear();
        for (int j = 0; j < covisN && j < (int)covis[k].size(); j++) {
            nb.push_back(&kfs[covis[k][j]]);
            cam.push_back(100 + covis[k][j]);
        }
    };
    std::ofstream ret(argv[3]);
    std::vector<sdm::KeyFrame*> nb;
    std::vector<int> cam;

    // only keyframe 0 reconstructed: its neighbours have no depth map yet
    pm.SemiDenseRecon(&kfs[0]);
    if (!pm.ok()) return 3;
    row(0, nb, cam);
    std::ostringstream none;
    ret << pm.AppendTranscriptEntryWithVisibility(&kfs[0], 100, nb, cam, none, 0.25) << " " << none.str().size() << std::endl;

    for (int k = 1; k < n_kf; k++) pm.SemiDenseRecon(&kfs[k]);
    // sizes differ
    row(0, nb, cam);
    cam.pop_back();
    ret << pm.AppendTranscriptEntryWithVisibility(&kfs[0], 100, nb, cam, none, 0.25) << " " << none.str().size() << std::endl;

    std::ofstream tr(argv[2]);
    for (int k = 0; k < n_kf; k++) {
        row(k, nb, cam);
        ret << pm.AppendTranscriptEntryWithVisibility(&kfs[k], 100 + k, nb, cam, tr, 0.25) << " "
            << (int)kfs[k].interKF_depth_flag_ << std::endl;
    }
    return 0;
}
