(ns raytrace-clj.gpu-lit-test
  "gpu/render-lit beside gpu/render, with an MI355X and librtmi.so on jna.library.path:

     lein test raytrace-clj.gpu-lit-test

   NEVER RUN where it was written (the build container has no JVM), like raytrace-clj.gpu-test."
  (:require [clojure.test :refer :all]
            [raytrace-clj.scene :as scene]
            [raytrace-clj.gpu :as gpu]))

(deftest ^:gpu render-lit-plain-is-the-frame
  ;; estimator 0 of gpu/render-lit traces the samples gpu/render traces, from camera rays built on the device: the same 8-bit frame and the same
  ;; segments.  make-two-spheres holds no light, so the light-sampled estimators are estimator 0 there and build no shadow ray.
  (let [sc  (scene/make-two-spheres 40 20)
        own (gpu/render sc 40 20 4)
        lit (gpu/render-lit sc 40 20 4 [] :estimator 0)
        mis (gpu/render-lit sc 40 20 4 [] :estimator 2 :light-choice 1)]
    (is (= (vec (:rgb8 lit)) (vec (:rgb8 own))))
    (is (= (:segments lit) (:total-rays own)))
    (is (= (* 40 20 4) (:total-rays lit)))
    (is (= (* 40 20 4 8) (count (:camera lit))))
    (is (= (vec (:linear mis)) (vec (:linear lit))))
    (is (zero? (:shadow-rays mis)))))

(deftest ^:gpu render-lit-refines-through-its-state
  ;; samples [0, 2) then [2, 4) through the returned state = samples [0, 4) in one call
  (let [sc   (scene/make-two-spheres 40 20)
        one  (gpu/render-lit sc 40 20 4 [] :estimator 0)
        a    (gpu/render-lit sc 40 20 2 [] :estimator 0)
        b    (gpu/render-lit sc 40 20 2 [] :estimator 0 :s-first 2 :state (:state a))]
    (is (= (vec (:linear b)) (vec (:linear one))))
    (is (= (vec (:stderr b)) (vec (:stderr one))))
    (is (= (+ (:segments a) (:segments b)) (:segments one)))))
